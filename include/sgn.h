/*
 * sgn.h — C ABI of libsgn, the MI355X-native packet-level network core for Shadow.
 *
 * libsgn replaces the data-parallel half of Shadow's simulation round (reference:
 * iiins0mn1a/shadow-gen, a Shadow 3.3.0 fork). Every entry point below names the
 * reference interface it replaces (file:line relative to the reference's src/main/ unless
 * stated). Conventions:
 *   - plain C types only, no torch/HIP types; caller owns every input array for the
 *     duration of the call, the library owns all device buffers;
 *   - every function returns int status: 0 = ok, negative = errno-style failure, with a
 *     message in sgn_last_error(ctx). Nothing unwinds or aborts across the ABI;
 *   - times are EmulatedTime nanoseconds (since the Unix epoch) unless a field says
 *     "_rel"/"_ns" (SimulationTime, nanoseconds since SIMULATION_START)
 *     (lib/shadow-shim-helper-rs/src/emulated_time.rs:25-50);
 *   - HostId is the u32 index of the host in hostname-sorted order (core/manager.rs:377-382).
 */
#ifndef SGN_H
#define SGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGN_ABI_VERSION 10

/* emulated_time.rs:27-40 */
#define SGN_SIMULATION_START 946684800000000000ULL
#define SGN_EMUTIME_INVALID 0xFFFFFFFFFFFFFFFFULL
#define SGN_EMUTIME_MAX 0xFFFFFFFFFFFFFFFEULL

/* core/definitions.h:124 */
#define SGN_CONFIG_MTU 1500u
/* IPv4 header (network/packet.rs:477-484) + UDP header (network/packet.rs:737-740) */
#define SGN_UDP_HEADER_BYTES 28u
/* IPv4 + TCP header: 20 B, plus the 3-B window-scale option padded to 4 (packet.rs:617-635) */
#define SGN_TCP_HEADER_BYTES 40u
#define SGN_TCP_WS_HEADER_BYTES 44u

/* status codes */
#define SGN_OK 0
#define SGN_EINVAL (-22)
#define SGN_ENOMEM (-12)
#define SGN_ENOENT (-2)
#define SGN_ERANGE (-34)
#define SGN_EDEVICE (-5)    /* HIP runtime failure */
#define SGN_ESTATE (-71)    /* call out of order (e.g. round before sim_init) */
#define SGN_EOVERFLOW (-75) /* a device capacity was exceeded; message names which */

typedef struct sgn_ctx sgn_ctx;

/* ------------------------------------------------------------------------------------ */
/* Context                                                                              */
/* ------------------------------------------------------------------------------------ */

typedef struct sgn_create_opts {
  int32_t device;      /* HIP device ordinal */
  uint32_t shard_rank; /* this process's shard (0 for a single GPU) */
  uint32_t shard_count;/* number of shards (1 for a single GPU) */
  uint32_t flags;      /* SGN_CREATE_* */
} sgn_create_opts;

#define SGN_CREATE_TIME_KERNELS 1u /* HIP events around the engine's launches (a sample: sgn_kernel_times) */
#define SGN_CREATE_TIME_EXECUTE 2u /* ... around the per-host execute kernel only */

/* Creates a context bound to one GPU. Replaces WorkerShared construction
 * (core/manager.rs:447-470) for the data-parallel state. */
int sgn_create(sgn_ctx** out, const sgn_create_opts* opts);
void sgn_destroy(sgn_ctx* ctx);
/* Last error message for ctx (or for a failed sgn_create when ctx == NULL). */
const char* sgn_last_error(const sgn_ctx* ctx);
/* ABI version compiled into the library. */
int sgn_abi_version(void);

/* ------------------------------------------------------------------------------------ */
/* Routing (network/graph/mod.rs:181-250, core/sim_config.rs:411-448)                   */
/* ------------------------------------------------------------------------------------ */

/* A parsed network graph: what NetworkGraph::parse (network/graph/mod.rs:132-179) produces.
 * Node i (0-based) is petgraph NodeIndex i; edges keep GML order. Self-loops are edges. */
typedef struct sgn_graph {
  uint32_t n_nodes;
  const uint32_t* node_id;          /* [n_nodes] GML ids */
  uint32_t n_edges;
  const uint32_t* edge_src;         /* [n_edges] GML ids */
  const uint32_t* edge_dst;         /* [n_edges] GML ids */
  const uint64_t* edge_latency_ns;  /* [n_edges] > 0 (graph/mod.rs:103) */
  const float* edge_loss;           /* [n_edges] in [0,1] (graph/mod.rs:99) */
  int32_t directed;
} sgn_graph;

/* Builds the U x U routing table {latency u64 ns, packet_loss f32} between the used nodes.
 * Replaces generate_routing_info (core/sim_config.rs:411) ->
 * NetworkGraph::compute_shortest_paths (graph/mod.rs:181) when use_shortest_path != 0, or
 * get_direct_paths (graph/mod.rs:228) otherwise. Entry (i,j) is the path from
 * used_node_ids[i] to used_node_ids[j]; (i,i) is the node's single self-loop edge
 * (graph/mod.rs:209-215). Errors (not aborts): unknown node, missing/duplicate self-loop,
 * disconnected used pair, missing/duplicate direct edge. */
int sgn_routes_build(sgn_ctx* ctx, const sgn_graph* graph, const uint32_t* used_node_ids,
                     uint32_t n_used, int32_t use_shortest_path);
/* RoutingInfo::path (graph/mod.rs:442) by GML node ids. SGN_ENOENT if not a used pair. */
int sgn_route_get(sgn_ctx* ctx, uint32_t src_node_id, uint32_t dst_node_id,
                  uint64_t* latency_ns, float* packet_loss);
/* Copies the whole table (row-major, used-node order) to host arrays of n_used^2 entries. */
int sgn_routes_copy(sgn_ctx* ctx, uint64_t* latency_ns, float* packet_loss);
/* RoutingInfo::get_smallest_latency_ns (graph/mod.rs:472): min over all U^2 entries. */
int sgn_min_latency(sgn_ctx* ctx, uint64_t* latency_ns);
/* Device time of the last sgn_routes_build (ms), split into its phases. */
typedef struct sgn_routes_timing {
  double total_ms;      /* whole build incl. upload/extract, device-timed */
  double latency_ms;    /* blocked min-plus (Floyd-Warshall) phase */
  double loss_ms;       /* tight-edge loss fold phase */
  uint32_t loss_iters;  /* sweeps to the fixed point */
  uint32_t tile;        /* min-plus tile edge T */
  uint64_t n_tight_edges;
  uint32_t latency_passes; /* min-plus squaring passes (u32 form), k-blocks (u64 Floyd-Warshall),
                              or relaxation sweeps (latency_bf) */
  uint32_t latency_u64;    /* 1: the u64 Floyd-Warshall form ran (an edge or path >= 2^32 - 1 ns) */
  uint32_t loss_multi;     /* sources per tight-arc sweep (u32 form, non-sparse graphs); 0: the
                              one-source loss pass */
  uint32_t latency_bf;     /* 1: sparse graph, latencies by per-source relaxation (u64, exact);
                              latency_passes = its most sweeps */
  uint32_t shards;         /* blocks the build was split into: the shard count when a
                              communicator is set (sgn_comm_init before the build; every shard
                              computes its block of used sources and the blocks are exchanged
                              over RCCL, so every shard ends with the whole table), else 1 */
  uint32_t shard_sources;  /* used sources whose rows this process computed */
  uint32_t loss_dense;     /* ABI 10: 1 when the sweep ran in its dense form (at least half of all
                              arcs, no parallel arcs: a (tail, head) matrix of arcs, loss_multi
                              sources per workgroup); 0: the CSR / arc-list sweep or none */
  uint32_t loss_fused;     /* ABI 10: 1 when the dense sweep ran fused with the first squaring pass
                              and found the direct arcs already closed (complete graphs whose arcs
                              are their own shortest paths): the tight arcs were found inside the
                              latency phase (latency_ms), and loss_ms is the fold alone */
} sgn_routes_timing;
int sgn_routes_timing_get(sgn_ctx* ctx, sgn_routes_timing* out);

/* ------------------------------------------------------------------------------------ */
/* Hosts (core/sim_config.rs:47-164,211-291; host/host.rs:234,283-295)                  */
/* ------------------------------------------------------------------------------------ */

typedef struct sgn_hosts {
  uint32_t n_hosts;            /* hosts in HostId order */
  const uint32_t* ip;          /* [n] IPv4 address, host byte order */
  const uint32_t* node_id;     /* [n] GML node id (must be a used node of the route table) */
  const uint64_t* bw_up_bits;  /* [n] HostInfo::bandwidth_up_bits (note sim_config.rs:252-254) */
  const uint64_t* bw_down_bits;/* [n] HostInfo::bandwidth_down_bits */
  const uint64_t* seed;        /* [n] HostInfo::seed = r ^ SipHash13(name) (sim_config.rs:242) */
} sgn_hosts;

/* Registers every host of the simulation (all shards pass the full list; each shard
 * keeps the contiguous HostId range it owns). Replaces DNS registration
 * (network/dns.rs:97-131: unspecified/loopback/broadcast/multicast and duplicate
 * addresses are errors) and Host::new's RNG/relay construction. */
int sgn_hosts_set(sgn_ctx* ctx, const sgn_hosts* hosts);

/* Derives per-host seeds exactly as SimConfig::new + build_host do
 * (core/sim_config.rs:50-54,220-242): G = Xoshiro256++::seed_from_u64(sim_seed);
 * r = G.next_u64(); seed[i] = r ^ SipHash13_{k0=k1=0}(names[i] || 0xFF). Host-side only. */
int sgn_derive_host_seeds(uint32_t sim_seed, const char* const* names, uint32_t n,
                          uint64_t* seeds_out);

/* ------------------------------------------------------------------------------------ */
/* Simulation rounds (core/manager.rs:541-656, host/host.rs:762-834, core/worker.rs:330-403)*/
/* ------------------------------------------------------------------------------------ */

typedef struct sgn_sim_config {
  uint64_t stop_time_ns;        /* general.stop_time (controller.rs:29-31) */
  uint64_t bootstrap_end_ns;    /* general.bootstrap_end_time (manager.rs:353-355) */
  uint64_t runahead_ns;         /* experimental.runahead; 0 = None (runahead.rs:55) */
  int32_t use_dynamic_runahead; /* experimental.use_dynamic_runahead (runahead.rs:61-67) */
  uint32_t out_fifo_cap;        /* synthetic socket send-queue entries per host (>= 1) */
  uint32_t codel_cap;           /* device CoDel run slots per host ON AVERAGE (reference:
                                   unlimited): the queues are chains of 16-run pages from one
                                   pool of max(hosts + 64, hosts * codel_cap / 16) pages, so any
                                   host may hold far more; exhausting the pool is
                                   SGN_EOVERFLOW, never a silent drop */
  uint32_t hosts_per_wave;      /* hosts served by one 64-lane execute wave: a power of two
                                   in [1, 64]; 0 = default (64). Performance only. */
  uint64_t event_capacity;      /* in-flight packet-event slots per shard (0 = auto) */
  uint32_t interface_qdisc;     /* experimental.interface_qdisc (configuration.rs:448,568,972):
                                   SGN_QDISC_FIFO (default) or SGN_QDISC_ROUND_ROBIN */
  uint32_t reserved;
} sgn_sim_config;

/* The interface's send queue of sockets (host/network/interface.rs:94-106,216-256,
 * queuing.rs:57-180). Every synthetic send-queue entry (a datagram, or a train written to its
 * own socket) is one socket. FIFO: sockets by the priority of their next packet = packets in
 * the order the applications wrote them. ROUND_ROBIN: the interface takes one packet from the
 * socket at the front and re-queues that socket at the back while it has more. */
#define SGN_QDISC_FIFO 0u
#define SGN_QDISC_ROUND_ROBIN 1u

/* Synthetic traffic (stands in for the managed processes, which stay on the CPU in
 * Shadow). Hosts talk UDP through the reference's own relay/router path. Workload
 * functions are defined once in sgn_workload.h. */
#define SGN_TRAFFIC_PERIODIC 1u /* configs B/D: every host sends one datagram per period */
#define SGN_TRAFFIC_TGEN 2u     /* config C: clients fetch files from servers as MTU trains */
#define SGN_TRAFFIC_EXTERNAL 3u /* no synthetic app: every host's application lives on the CPU;
                                   its datagrams enter with sgn_submit and its deliveries and
                                   drops leave with sgn_drain (the mixed real-app mode) */

typedef struct sgn_traffic {
  uint32_t kind;
  uint32_t payload_len;          /* PERIODIC datagram payload bytes */
  uint64_t flow_seed;
  uint64_t start_ns;             /* first app event (sim time) */
  uint64_t start_jitter_ns;      /* + H(i) % (jitter + 1) */
  uint64_t period_ns;            /* PERIODIC send period / TGEN think time */
  uint64_t period_jitter_ns;     /* TGEN: think time + H % (jitter + 1) */
  uint32_t unknown_dst_permille; /* PERIODIC: sends to an address outside the simulation */
  uint32_t req_payload;          /* TGEN request datagram payload */
  uint32_t n_servers;            /* TGEN */
  uint32_t reserved0;
  const uint32_t* server_hosts;  /* TGEN [n_servers] HostIds of servers (ascending) */
  uint64_t file_bytes[3];        /* TGEN file sizes (e.g. 50 KiB, 1 MiB, 5 MiB) */
} sgn_traffic;

/* Uploads state and schedules each host's first app event. Must follow routes_build and
 * hosts_set. Host RNGs are Xoshiro256++::seed_from_u64(seed) (host/host.rs:234). */
int sgn_sim_init(sgn_ctx* ctx, const sgn_sim_config* cfg, const sgn_traffic* traffic);

/* The current window [start, end) (EmulatedTime). The first is
 * [SIMULATION_START, SIMULATION_START + 1 ns) (manager.rs:506-509). active = 0 once
 * Controller::manager_finished_current_round returned None (controller.rs:88-112). */
int sgn_window(sgn_ctx* ctx, uint64_t* start, uint64_t* end, int32_t* active);

/* Runs one round on the current window: every owned host executes its events with
 * time < end (Host::execute, host.rs:762-830), packets are routed (Worker::send_packet,
 * worker.rs:330-403), events are queued at their destinations (push_packet_to_host,
 * worker.rs:603-613), then min_next_event = min over all queue heads (manager.rs:580-628)
 * and the next window is computed on the device. Synchronous. */
int sgn_round(sgn_ctx* ctx, uint64_t* min_next_event);

/* Runs up to max_rounds rounds without a host synchronisation per round (rounds are
 * enqueued in batches; the window lives on the device). Stops early when the simulation
 * ends. rounds_done may be NULL. */
int sgn_run(sgn_ctx* ctx, uint64_t max_rounds, uint64_t* rounds_done);

/* ---- run-control: run to a simulated time, snapshot, rewind ----
 * The reference fork's run-control (core/manager.rs:49-111, :1117-1442) pauses at window
 * boundaries, runs one window (n), runs N simulated seconds (cN), and restarts (r, rN) — by
 * re-running from t = 0, because its state is live Linux processes. Here a simulation is device
 * buffers plus a few host counters and the engine is bit-deterministic, so a snapshot is exact:
 *   n  = sgn_run(ctx, 1, ..)                 s  = sgn_hosts_next_event_time
 *   cN = sgn_run_until(ctx, now + N, ..)     rN = sgn_snapshot_restore(first) + sgn_run_until(N)
 * These calls are single-shard: a context created with shard_count > 1 or joined to a local
 * shard group gets SGN_ESTATE from them, because a multi-shard snapshot or pause needs a
 * collective over every shard at one round edge — the sgn_shards_* calls below. */

/* Runs whole windows until the next window would start at or after t_emulated (EmulatedTime,
 * i.e. SGN_SIMULATION_START + simulated ns), or the simulation ends — the fork's rule "pause
 * when min_next_event_time >= target" (manager.rs:1372-1382). t_emulated at or below the current
 * window start runs nothing (rounds_done = 0). The comparison runs on the device at every round
 * edge, so persistent launches still run many rounds each; sgn_run and sgn_round never pause.
 * rounds_done may be NULL.
 * With SGN_TRAFFIC_EXTERNAL traffic the call runs the datagrams already submitted: before
 * running to t_emulated, submit every datagram with send_time < t_emulated + the longest window
 * (see sgn_submit, "Submitting ahead"); the call returns early, inactive, when the device has
 * no event left, and sgn_set_window + sgn_submit continue from there. */
int sgn_run_until(sgn_ctx* ctx, uint64_t t_emulated, uint64_t* rounds_done);

/* A snapshot of the simulation. Opaque; owned by the context it came from (sgn_snapshot_free, or
 * sgn_destroy for what is left). A context may hold any number of them and restore them in any
 * order, any number of times. */
typedef struct sgn_snapshot sgn_snapshot;

/* Saves the simulation as it is now. Valid after sgn_sim_init, between calls, at a resolved
 * round edge: a round still held for a pool (or runs in the calendar's spill area) is resolved
 * first, as sgn_run does on entry, and CPU-held host RNG states (sgn_rng_*) go back to the device
 * before they are copied. It does not change the simulation: a run with a save in the middle is
 * bit-identical to one without. The event calendar is stored packed (its live runs only), every
 * other mutable buffer whole. SGN_ENOMEM leaves nothing behind. */
int sgn_snapshot_save(sgn_ctx* ctx, sgn_snapshot** out);

/* Puts the context back into exactly the state at the save: the device state, the host-side
 * simulation state (rounds enqueued, submission handles and per-host submission counts, drain
 * records held for the caller, slab extensions), the growth counters sgn_engine_info reports
 * (codel_pool_grows, calendar_grows, calendar_spill_runs, slab_extensions, spill_area_grows,
 * rounds_held, codel_page_allocs), and the pool layout: pools that grew after the save (slab
 * capacity, slab extensions, CoDel pages, spill area) return to the saved sizes, so the run after
 * a restore grows them again at the same rounds. CPU-held RNG states are dropped.
 * NOT rewound, because they belong to the sequence of launches and not to the simulation: the
 * persistent kernels' residency census and epochs, persistent_grid's fallback state
 * (persistent_fallbacks), and the kernel-time samples of sgn_kernel_times (measurements).
 * Trace records are append-only: restore sets the record count back and the re-run writes the
 * same records again. Drain records the caller already took with sgn_drain stay the caller's;
 * records still on the device or held at the save come back.
 * A snapshot saved here keeps no trace records — those up to its save are in the trace buffer — so
 * one AHEAD of the position (the run was rewound behind it) restores only while they are still
 * there: the records past the position stay in place until the cursor of sgn_trace_take moves (a
 * take, or a restore that takes the cursor back), and come back when the run passes the snapshot's
 * round again. Otherwise SGN_ESTATE, nothing changed; sgn_snapshot_export follows the same rule, and
 * an imported snapshot carries its records and always restores.
 * Errors: SGN_EINVAL for a null argument or a snapshot that is not this context's; SGN_ESTATE
 * without a simulation, for a snapshot taken before the last sgn_sim_init, or for one whose trace
 * records left the buffer (above); SGN_ENOMEM with nothing changed. */
int sgn_snapshot_restore(sgn_ctx* ctx, const sgn_snapshot* snap);

/* Frees one snapshot (a null argument, or a snapshot that is not this context's: no effect). */
void sgn_snapshot_free(sgn_ctx* ctx, sgn_snapshot* snap);

typedef struct sgn_snapshot_info {
  uint64_t rounds, window_start, window_end; /* the round count and window at the save */
  uint64_t device_bytes, host_bytes;         /* what the snapshot holds */
  uint64_t calendar_runs, calendar_bytes;    /* packed section: runs and their bytes (32 each) */
  uint64_t calendar_pool_bytes;              /* the unpacked pool + extensions it stands for */
  double save_ms;                            /* HIP-event time of the device part of the save */
  double pack_ms;                            /* ... of which the calendar's scan + pack kernels */
} sgn_snapshot_info;
int sgn_snapshot_info_get(const sgn_snapshot* snap, sgn_snapshot_info* out);

/* ---- run-control for sharded simulations ----
 * ctxs: THIS process's shards — all n contexts of a local group (rank order), or the one context
 * of a rank that has a communicator (n = 1). In the second form every rank makes the same call
 * with the same arguments at the same round edge: a collective. Anything else (a part of a
 * group, an unsharded context) is SGN_ESTATE; a null pointer is SGN_EINVAL.
 *   n  = sgn_run / sgn_run_local_group(.., 1, ..)     cN = sgn_shards_run_until(now + N)
 *   r  = sgn_shards_snapshot_restore(first)           rN = r + sgn_shards_run_until(N)
 *
 * sgn_shards_run_until follows sgn_run_until's rule exactly: every shard pauses at the first
 * round edge whose next window starts at or after t_emulated (the multi-shard round edges compute
 * that window from the same N messages on every shard, so all shards pause at the same edge, on
 * the device); a target at or below the current window start, or an ended simulation, runs
 * nothing. rounds_done (may be NULL): the rounds every shard ran. Ranks that pass different
 * targets all get SGN_EINVAL before anything is launched. */
int sgn_shards_run_until(sgn_ctx* const* ctxs, uint32_t n, uint64_t t_emulated, uint64_t* rounds_done);

/* One snapshot per shard, all of the same resolved round edge (a round still held — a pool, a
 * re-layout, runs waiting for a larger inbox — is resolved across the shards first). out[i] is
 * owned by ctxs[i]; sgn_snapshot_free and sgn_snapshot_info_get apply to it. All or nothing: on
 * any failure every snapshot taken in the call is freed and out[] is all NULL. */
int sgn_shards_snapshot_save(sgn_ctx* const* ctxs, uint32_t n, sgn_snapshot** out /* [n] */);

/* Every shard back to snaps[i], as sgn_snapshot_restore does for one: the shard's own state and
 * pools (slab capacity, extensions, CoDel pages, spill area) return to the saved sizes. The one
 * deliberate difference is the exchange layer, which belongs to the sequence of launches: inboxes
 * and exchange slots keep the sizes they have grown to (inbox_slot_runs, exchange_slot_runs and
 * exchange_send_runs do not shrink; no output depends on them), and the transport counters
 * (inbox_grows, exchange_slot_grows, exchange_spills, inbox_overflow_rounds, inbox_moved_runs,
 * exchange_bytes, persistent_x_launches) are not rewound.
 * Everything is checked before anything changes: SGN_EINVAL when snaps[i] is null, is not
 * ctxs[i]'s, or the snapshots are of different rounds; SGN_ESTATE for a snapshot taken before
 * the last sgn_sim_init. */
int sgn_shards_snapshot_restore(sgn_ctx* const* ctxs, uint32_t n, sgn_snapshot* const* snaps /* [n] */);

/* ---- snapshot files: a snapshot out of its context and process, and back into a fresh one ----
 * The reference has no checkpoint (a restart re-runs from t = 0). A snapshot's state is
 * pointer-free, so a file is a matter of format and validation: a header (what wrote it, which
 * simulation, the round edge, the pool layout), a table {id, bytes, digest} of sections, the
 * sections (every device buffer of the snapshot, the packed calendar, the host-side vectors, the
 * trace records up to the save), and a trailer digest over header and table. Little-endian, every
 * section padded to 16 bytes. A file belongs to the library build that wrote it — it is not an
 * interchange format — and to one simulation: the header carries an IDENTITY digest of the route
 * table, every host's constants (address, node, bandwidths, seed), the sgn_sim_config and
 * sgn_traffic fields (server list included), the shard rank, count and owned range, and the
 * calendar's shape; the same calls in another process give the same identity. */
#define SGN_EFILE (-74) /* a snapshot file is truncated, corrupt, or a stream callback failed */

/* Stream callbacks: called in order, never asked to seek. Return 0 when all len bytes were
 * written / filled; anything else ends the call with SGN_EFILE. */
typedef int (*sgn_write_fn)(void* user, const void* data, size_t len);
typedef int (*sgn_read_fn)(void* user, void* data, size_t len);

/* Writes snap (owned by ctx, of the current sgn_sim_init: else the errors of sgn_snapshot_restore)
 * in one forward pass: header and table, the sections, the trailer. Neither the simulation nor the
 * snapshot changes. Device sections are digested on the device before they leave and stream
 * through two pinned staging chunks, so host memory stays bounded whatever the snapshot's size.
 * Trace records [b, min(trace count at the save, b + capacity)) are taken from the context's trace
 * buffer (the engine is deterministic: they are still there — or, for a snapshot ahead of the
 * position after the cursor moved, SGN_ESTATE as for sgn_snapshot_restore), b the records
 * sgn_trace_take has handed out, 0 without a take; the header carries b. bytes (may be NULL): the
 * file's length. */
int sgn_snapshot_export(sgn_ctx* ctx, const sgn_snapshot* snap, sgn_write_fn write, void* user, uint64_t* bytes);

/* Builds a new snapshot owned by ctx from a stream, as if sgn_snapshot_save had just taken it here
 * — and does nothing else: the simulation is untouched until sgn_snapshot_restore (or
 * sgn_shards_snapshot_restore: every shard imports its own file, no collective needed) is called
 * with it. Needs a simulation made by the same calls as the exporter's (SGN_ESTATE without one).
 * All or nothing: on any failure every buffer is freed and *out is NULL.
 * Errors: SGN_EINVAL when a header field differs from this library or this simulation (the
 * message names the field; another identity is one of them); SGN_EFILE for a truncated stream, a
 * section whose size does not follow from the simulation and the header, a section or trailer
 * digest that does not match (sections are digested again on the device after the upload; the
 * message names the section), or slab fills that disagree with the packed calendar's run count;
 * SGN_ESTATE for a file with trace records into a context without a trace buffer that holds them
 * (or the reverse). The imported snapshot carries its trace records and a restore writes them
 * back; sgn_snapshot_info_get reports the saved round, window, sizes and runs, save_ms = pack_ms
 * = 0. */
int sgn_snapshot_import(sgn_ctx* ctx, sgn_read_fn read, void* user, sgn_snapshot** out);

/* The same through a file: export writes path + ".tmp" and renames it on success (a failure
 * removes the temporary file and leaves path alone); import reads path (SGN_ENOENT: cannot open). */
int sgn_snapshot_export_file(sgn_ctx* ctx, const sgn_snapshot* snap, const char* path, uint64_t* bytes);
int sgn_snapshot_import_file(sgn_ctx* ctx, const char* path, sgn_snapshot** out);

/* A file's header: no device call, no context. SGN_ENOENT when path cannot be opened, SGN_EFILE
 * when it is shorter than its header says, has another magic, or its trailer digest fails. */
typedef struct sgn_snapshot_file_info {
  uint64_t format, abi, layout_sig, identity; /* what wrote it, and which simulation */
  uint64_t rounds, window_start, window_end;  /* the round edge */
  uint64_t file_bytes, n_sections, calendar_runs, trace_records;
  uint32_t shard_rank, shard_count;
} sgn_snapshot_file_info;
int sgn_snapshot_file_info_get(const char* path, sgn_snapshot_file_info* out);

/* Whole-simulation counters (summed over owned hosts). */
typedef struct sgn_stats {
  uint64_t rounds;
  uint64_t packets_sent;       /* send_packet executions that passed the DNS check */
  uint64_t packets_loss_dropped;/* ... of which dropped by path reliability (worker.rs:371) */
  uint64_t packets_unknown_dst;/* InetDropped: destination not in the simulation (:347) */
  uint64_t packet_events_popped;/* packet events executed at destinations (host.rs:797) */
  uint64_t codel_dropped;      /* RouterDropped by CoDel (codel_queue.rs:319) */
  uint64_t delivered;          /* inbound packets handed to the host interface */
  uint64_t local_delivered;    /* packets to the host's own address (relay is_local) */
  uint64_t app_blocked;        /* synthetic sends refused by a full send queue */
  uint64_t local_events;       /* local (task) events executed */
  uint64_t bytes_delivered;    /* payload bytes handed to the interface */
  uint64_t min_used_latency_ns;/* Runahead::min_used_latency, SGN_EMUTIME_INVALID if none */
  uint64_t max_codel_len;      /* high-water mark of any CoDel ring (capacity planning) */
  uint64_t max_pending_events; /* high-water mark of in-flight packet events */
  uint64_t host_executions;    /* sum over rounds of hosts that had an event due */
  uint64_t sched_heavy_hosts;  /* sum over rounds of hosts run on a wave of their own */
  uint64_t sched_sorted_segments; /* sum over rounds of per-host segments that needed sorting */
  uint64_t event_runs;         /* due event runs (records) processed; <= packet_events_popped */
} sgn_stats;
int sgn_stats_get(sgn_ctx* ctx, sgn_stats* out);

/* Per-host order-sensitive digests (sgn_workload.h: SGN_DIGEST_*), counters and final RNG
 * state for the owned range [host_lo, host_hi). Arrays hold (host_hi - host_lo) entries;
 * any pointer may be NULL. Used by parity tests at full sizes. */
typedef struct sgn_host_digest {
  uint64_t tx;        /* every send_packet outcome, in order */
  uint64_t rx;        /* every packet event popped, in order (event order proof) */
  uint64_t app;       /* every interface delivery / CoDel drop, in order */
  uint64_t rng[4];    /* Xoshiro256++ state */
  uint64_t next_event_id;
  uint64_t n_sent, n_popped, n_delivered, n_codel_dropped;
} sgn_host_digest;
int sgn_host_digests(sgn_ctx* ctx, uint32_t host_lo, uint32_t host_hi, sgn_host_digest* out);

/* Host::next_event_time (host.rs:832): backs worker_maxEventRunaheadTime (worker.rs:774).
 * SGN_EMUTIME_INVALID when the queue is empty. Only valid between rounds. */
int sgn_host_next_event_time(sgn_ctx* ctx, uint32_t host, uint64_t* t);
/* The same for every owned host in [host_lo, host_hi) at once (out[host - host_lo]): one
 * device pass over the host records and the calendar, one copy. A CPU controller reads its
 * hosts' worker_maxEventRunaheadTime inputs with one call per round, not one per host. */
int sgn_hosts_next_event_time(sgn_ctx* ctx, uint32_t host_lo, uint32_t host_hi, uint64_t* out);

/* Per-packet trace (for bit-exact comparison at small sizes). Enable before sim_init.
 * The record kinds follow a packet through the path:
 *   IF_POP   the interface hands a packet to relay_inet_out (NetworkInterface::pop,
 *            interface.rs:216-256 - the pcap capture point of a sent packet, interface.rs:192-215)
 *   SEND     Worker::send_packet's outcome (worker.rs:330-403)
 *   POP      the packet event runs at its destination (host.rs:762-830)
 *   DELIVER  the interface receives it (NetworkInterface::push - the receive capture point)
 *   LOCAL    a packet to the host's own address, pushed back into the interface (relay/mod.rs:84-87)
 *   CODEL_DROP the router's CoDel queue drops it (codel_queue.rs:319-321)
 * b of IF_POP / DELIVER / LOCAL = payload | tag << 32 (the header kind rides in the tag). */
#define SGN_TRACE_SEND 1u   /* a = now, b = deliver time (0 if dropped/unknown), c = event id */
#define SGN_TRACE_POP 2u    /* a = event time, b = 0, c = src event id */
#define SGN_TRACE_DELIVER 3u/* a = now, b = payload|tag<<32, c = src event id */
#define SGN_TRACE_CODEL_DROP 4u
#define SGN_TRACE_IF_POP 5u /* a = now, b = payload|tag<<32, c = dst address when peer is unknown */
#define SGN_TRACE_LOCAL 6u  /* a = now, b = payload|tag<<32 */
typedef struct sgn_trace_rec {
  uint32_t kind;     /* SGN_TRACE_* */
  uint32_t host;     /* host where it happened */
  uint32_t peer;     /* SEND / IF_POP: dst HostId (0xFFFFFFFF unknown); LOCAL: itself; others: src HostId */
  uint32_t flags;    /* SEND: 0 sent, 1 loss-dropped, 2 unknown dst */
  uint64_t a, b, c;
  uint64_t seq;      /* per-host sequence number of this record */
  uint64_t rng_pos;  /* the host RNG's stream position: draws made so far, this record's
                        loss draw included (host.rs:234; worker.rs:366 draws one per
                        send_packet past the DNS check; sgn_rng_* draws count too) */
} sgn_trace_rec;
int sgn_trace_enable(sgn_ctx* ctx, uint64_t capacity);
/* Copies up to cap records (unordered; sort by (host, seq)). n_total = records produced. After
 * sgn_trace_take (below) the copy holds the records still in the buffer: those produced since
 * the last take. */
int sgn_trace_read(sgn_ctx* ctx, sgn_trace_rec* out, uint64_t cap, uint64_t* n_total);

/* ---- additions to ABI 10 (new calls only; no struct of ABI 10 changes): a trace of chosen hosts,
 * taken out in ordered pieces while the simulation runs. The reference's only network-level
 * output is the per-host capture (host_options.pcap_enabled, pcap_capture_size:
 * core/configuration.rs:602-621, interface.rs:192-215); with these calls a capture of a few hosts
 * of a large, long run needs a trace buffer for one interval only. ----
 *
 * sgn_trace_hosts: after sgn_trace_enable and before sgn_sim_init (SGN_ESTATE otherwise), the
 * HostIds whose records the trace keeps, in any order; only they produce records, advance seq and
 * keep rng_pos, and their records are exactly those of an unrestricted trace of the same
 * simulation (every field). A repeated id is SGN_EINVAL here, an id >= n_hosts SGN_EINVAL at
 * sgn_sim_init. n = 0 removes the set (every host is traced). Every shard of a sharded run passes
 * the same list and records the hosts it owns. The set is part of a snapshot file's identity when
 * one is given. */
int sgn_trace_hosts(sgn_ctx* ctx, const uint32_t* hosts, uint32_t n);

/* Records produced and not yet taken. */
int sgn_trace_pending(sgn_ctx* ctx, uint64_t* n);

/* One host's records inside a take: out[first .. first + count). */
typedef struct sgn_trace_span {
  uint32_t host, reserved;
  uint64_t first, count;
} sgn_trace_span;

/* Between calls (like sgn_drain): moves every record produced and not yet taken into out, sorted
 * by (host, seq) on the device, and empties the trace buffer — its whole capacity is free again,
 * so sgn_trace_enable's capacity need only hold what one interval between two takes produces
 * (more is SGN_EOVERFLOW at the round, as without takes). spans (may be NULL) gets one entry per
 * host with records, ascending by host. All or nothing: with cap below the pending count, or
 * span_cap below the hosts with records, SGN_ERANGE, *n_out and *n_spans say what is needed and
 * nothing is taken. The simulation does not change (window, counters and digests are those of a
 * run without takes). SGN_EDEVICE when a host's pending records do not carry consecutive seq (the
 * message names the host; nothing is taken).
 * Snapshots: sgn_snapshot_restore sets the records produced back to the save's count N, and the
 * taken count too when it was above N — the re-run produces those records again and they are taken
 * again (the rule of drain records the caller already took). sgn_snapshot_export writes the
 * records [b, N) still held, b = min(taken, N); the file's header carries b, and a restore of the
 * imported snapshot leaves exactly those pending (the importing context's buffer must hold N - b
 * records). */
int sgn_trace_take(sgn_ctx* ctx, sgn_trace_rec* out, uint64_t cap, uint64_t* n_out, sgn_trace_span* spans,
                   uint64_t span_cap, uint64_t* n_spans);

/* What the context's last sgn_trace_take spent (measurements; tools/capture_timing.py). */
typedef struct sgn_trace_take_timing {
  double total_ms;      /* wall time of the call */
  double kernel_ms[3];  /* HIP-event times: per-host count and seq range, scan and spans, scatter */
  double copy_ms;       /* HIP-event time of the device-to-host copies */
  uint64_t records, hosts;
} sgn_trace_take_timing;
int sgn_trace_take_timing_get(sgn_ctx* ctx, sgn_trace_take_timing* out);

/* ---- additions to ABI 10 (new calls only; no struct of ABI 10 changes): interval statistics —
 * what every owned host sent, received and dropped between two samples, read on the device. The
 * reference has no such output (its only network-level output is the per-host capture above); a
 * caller that wanted it had to read sgn_host_digests and sgn_stats_get at every pause, which copy
 * every host record to the CPU. A sample compares the seven per-host counters behind those two
 * calls with a device-resident baseline and keeps one row per host that changed. The sampler
 * stands beside the simulation: it reads the counters at a launch boundary and never changes
 * window, counters, digests or any snapshot. ---- */

typedef struct sgn_sample_row {   /* 64 B: one host's activity between two samples */
  uint32_t host;                  /* HostId */
  uint32_t sample;                /* index of the sample that closed the interval (its low 32 bits) */
  uint64_t sent, popped, delivered, codel_dropped,   /* deltas of the counters behind sgn_host_digest */
           unknown_dst, local_delivered, blocked;    /* ... and behind sgn_stats' per-host sums */
} sgn_sample_row;

typedef struct sgn_sample_info {  /* one per sample */
  uint64_t sample, rounds, window_start, window_end; /* the round edge it was taken at (sgn_window) */
  uint64_t first_row, rows;       /* its rows inside a take: out[first_row .. first_row + rows) */
  uint64_t total[7];              /* sum of its rows' seven deltas (the rows' field order), folded on
                                     the device */
} sgn_sample_info;

/* After sgn_sim_init, between calls: allocates a device buffer of row_capacity rows and a device
 * baseline of seven u64 per owned host, set to the counters as they are now. The sample index
 * starts at 0. A second call re-allocates and rebases: pending rows and samples are dropped and
 * the index starts at 0 again. A new sgn_sim_init drops the sampler. row_capacity == 0 is
 * SGN_EINVAL; SGN_ENOMEM leaves the context without a sampler. */
int sgn_sample_enable(sgn_ctx* ctx, uint64_t row_capacity);

/* Between calls, at whatever round edge the context is at (typically after sgn_run_until); no
 * held round is resolved, the per-host counters are final at every launch boundary. For every
 * owned host with any of the seven counters differing from the baseline it appends one row
 * (current - baseline) to the device row buffer, rows ascending by HostId, sets that host's
 * baseline to the current values, and records the sample's info (*out, when given, is that info
 * with first_row = the rows pending before the call). Hosts without a change produce no row; a
 * sample without rows is still a sample (rows = 0, the index advances).
 * All or nothing: with fewer free rows than the sample needs, SGN_EOVERFLOW (the message says how
 * many it needs and how many are free), nothing is appended, baseline and index are unchanged,
 * and the same call succeeds after a sgn_sample_take.
 * Works on any context — members of a local group and ranks with a communicator included: it
 * samples the hosts the context owns and is not a collective.
 * Rewinds: the sampler is not part of a snapshot and sgn_snapshot_restore /
 * sgn_shards_snapshot_restore leave it alone. When the context's round count is below the round
 * count of the baseline (the deltas would be negative) the call returns SGN_ESTATE and nothing
 * changes; it keeps returning SGN_ESTATE until sgn_sample_rebase. */
int sgn_sample(sgn_ctx* ctx, sgn_sample_info* out /* may be NULL */);

/* Sets the baseline to the current counters. Emits nothing; pending rows, pending samples and the
 * sample index stay as they are. */
int sgn_sample_rebase(sgn_ctx* ctx);

/* Rows and samples appended and not yet taken (either pointer may be NULL). */
int sgn_sample_pending(sgn_ctx* ctx, uint64_t* rows, uint64_t* samples);

/* Like sgn_trace_take: moves every pending row (ordered by sample, then host) out in one
 * device-to-host copy, the pending samples' infos with them, and empties the buffer. With cap
 * below the pending rows or info_cap below the pending samples, SGN_ERANGE, *n_out and *n_infos
 * say what is needed and nothing is taken. infos may be NULL (info_cap 0) only when no sample is
 * pending; n_infos may be NULL. */
int sgn_sample_take(sgn_ctx* ctx, sgn_sample_row* out, uint64_t cap, uint64_t* n_out,
                    sgn_sample_info* infos, uint64_t info_cap, uint64_t* n_infos);

/* What the context's last sgn_sample spent (measurements; tools/sample_timing.py): the wall time
 * of the call, the HIP-event times of its three kernels (per-wave count of changed hosts, scan,
 * scatter of rows + baseline update + totals), its owned hosts and rows; copy_ms is the
 * HIP-event time of the last sgn_sample_take's device-to-host copy of rows (0 before one).
 * Errors in common for the six calls: a null context SGN_EINVAL; no simulation, or the sampler not
 * enabled, SGN_ESTATE; a HIP failure SGN_EDEVICE. */
typedef struct sgn_sample_timing { double total_ms, kernel_ms[3], copy_ms; uint64_t hosts, rows; } sgn_sample_timing;
int sgn_sample_timing_get(sgn_ctx* ctx, sgn_sample_timing* out);

/* ---- additions to ABI 10 (new calls only; no struct of ABI 10 changes): the backlog report —
 * what is STANDING in the network at a round edge, per owned host: the packets in its router's
 * CoDel queue and the age of the queue's head, what waits in its socket send queue behind the
 * uplink token bucket, and the packets in flight towards it. Traces, captures and samples report
 * what has flowed; sgn_stats only has the high-water marks max_codel_len and max_pending_events.
 * The state is on the device and final at every launch boundary (host records, CoDel page pool,
 * send-queue rings, event calendar); the report reads it there and stands beside the simulation
 * like sgn_sample: it writes scratch of its own and nothing else. ---- */

#define SGN_BACKLOG_ROUTER_HELD 1u /* relay_inet_in holds one packet taken from the CoDel queue, waiting for tokens */
#define SGN_BACKLOG_OUT_HELD    2u /* relay_inet_out holds one packet taken from the interface (IF_POP recorded), not yet sent */

typedef struct sgn_backlog_row {          /* 64 B, one per owned host with anything standing */
  uint32_t host, flags;                   /* HostId; SGN_BACKLOG_* */
  uint32_t router_packets, send_packets;  /* CoDel queue / socket send queue, the held packets NOT included */
  uint64_t router_bytes;                  /* CoDel's total_bytes (wire bytes, as CoDelQueue keeps them) */
  uint64_t send_bytes;                    /* wire bytes of the send queue: payload + sgn_header_bytes(tag) per packet */
  uint64_t router_oldest;                 /* enqueue time of the CoDel queue's head (EmulatedTime); SGN_EMUTIME_INVALID when empty */
  uint32_t inflight_packets;              /* packets in the calendar addressed to this host */
  uint32_t submit_pending;                /* EXTERNAL: submitted datagrams of this host not yet reached (0 otherwise) */
  uint64_t inflight_earliest, inflight_latest; /* their delivery times; INVALID / 0 when none */
} sgn_backlog_row;

typedef struct sgn_backlog_info {
  uint64_t rounds, window_start, window_end;  /* the round edge (sgn_window) */
  uint64_t hosts, rows;                       /* owned hosts; hosts with a row */
  uint64_t total[8];  /* router_packets, router_bytes, router_held, send_packets, send_bytes, out_held, inflight_packets, submit_pending */
  uint64_t max_router_packets;  uint32_t max_router_host, pad0;
  uint64_t max_sojourn_ns;      uint32_t max_sojourn_host, pad1;  /* window_start - router_oldest, its largest */
  uint64_t inflight_earliest;   /* min over rows; INVALID when nothing is in flight */
} sgn_backlog_info;

/* After sgn_sim_init, between calls, at whatever round edge the context is at (typically after
 * sgn_run_until); on a finished simulation it reports what is left. A host gets a row when it has
 * a flag, a packet or a byte in either queue, a packet in flight towards it or a submitted datagram
 * pending (router_oldest and inflight_earliest are SGN_EMUTIME_INVALID for a host without either, so
 * they alone make no row); rows ascend by HostId. info->total sums the rows' fields (router_held /
 * out_held: rows with that flag); the maxima are over the hosts with a non-empty CoDel queue, on
 * equal values the lowest HostId, 0 / host 0 when no queue holds a packet. Totals and maxima are
 * folded on the device.
 * out == NULL with cap == 0 asks for the totals only: SGN_OK, info filled, *n_out = the row count,
 * no row copied. With out != NULL and cap below the row count: SGN_ERANGE, *n_out says what is
 * needed, info is filled and nothing is written to out.
 * Read-only: window, counters, digests, traces, drain records, sampler and snapshots are what they
 * would be without the call. Its scratch is allocated on first use, sized by the owned hosts, and
 * freed by sgn_destroy or a new sgn_sim_init.
 * Held rounds. On a single-shard context a round held for a pool, or runs in the calendar's spill
 * area, are resolved first, exactly as sgn_snapshot_save does; afterwards every pending event is in
 * a slab or its extension. A member of a local group or a rank with a communicator cannot resolve
 * a held edge alone: there the call returns SGN_ESTATE with nothing read (the next collective run
 * or save call resolves it). At a resolved edge it reports the hosts the context owns, like
 * sgn_sample, and is not a collective; in-flight packets are counted at the shard that owns the
 * destination (at a launch's end the imports are filed).
 * Errors: null ctx, n_out or info (or out == NULL with cap != 0) SGN_EINVAL; no simulation
 * SGN_ESTATE; a HIP failure, or calendar words that point outside the calendar, SGN_EDEVICE. */
int sgn_backlog(sgn_ctx* ctx, sgn_backlog_row* out, uint64_t cap, uint64_t* n_out, sgn_backlog_info* info);

/* What the context's last sgn_backlog spent (measurements; tools/backlog_timing.py): the wall time
 * of the call, the HIP-event times of its four kernels (calendar pass, per-wave count of hosts
 * with a row, scan, scatter of rows + totals), of the device-to-host copy of the rows (0 for the
 * totals-only form), its owned hosts and rows, and the calendar runs the first kernel read.
 * SGN_ESTATE before the first sgn_backlog of the simulation. */
typedef struct sgn_backlog_timing { double total_ms, kernel_ms[4], copy_ms; uint64_t hosts, rows, calendar_runs; } sgn_backlog_timing;
int sgn_backlog_timing_get(sgn_ctx* ctx, sgn_backlog_timing* out);

/* ------------------------------------------------------------------------------------ */
/* CPU-resident applications (SGN_TRAFFIC_EXTERNAL)                                      */
/* ------------------------------------------------------------------------------------ */

/* Packet ingress: datagrams written by CPU-side applications (the socket send that ends in
 * Host::notify_socket_has_packets, host.rs:969-983, and then relay_inet_out + Router::push +
 * Worker::send_packet, worker.rs:330). Each datagram is queued on the device as an event of
 * its source host at send_time; when the host reaches it (ordered with the host's packet
 * events at that time by (source = itself, submission order)), it enters the host's socket
 * send queue and the relay path takes it from there exactly like a synthetic app's datagram
 * (token bucket, loss draw from the device-held host RNG, source event id, delivery time).
 * Rules: traffic kind SGN_TRAFFIC_EXTERNAL; src_host owned by this shard; send_time in
 * [current window start, stop time) and within the event calendar's horizon (the
 * longest route latency ahead of the window); payload_len <= 65535; wire_len 0 or
 * payload_len + 28 (UDP over IPv4, packet.rs:388-396,477-484,737-740), or payload_len + 40 /
 * + 44 (a TCP segment from the CPU TCP stack without / with the window-scale option,
 * packet.rs:617-635; the wire length feeds the token buckets and CoDel's byte count, and a
 * zero-payload segment is never loss-dropped, worker.rs:371). handle is opaque
 * (the payload stays on the CPU) and comes back in the packet's drain record. Call between
 * rounds; a failed call queues nothing. Replaces Worker::send_packet's CPU callers.
 *
 * Submitting ahead. A controller need not submit window by window: any send_time below the
 * horizon — window start + (calendar_buckets - 2) * bucket_width_ns, both from
 * sgn_engine_info_get — is accepted, and sgn_run / sgn_run_until / sgn_run_local_group /
 * sgn_shards_run_until then run many rounds per call (the persistent round kernels) with the
 * datagrams taken at their times; windows and fates are those of submitting each window's
 * datagrams just before its round. What must be in before running to a time T: every datagram
 * with send_time < T + the longest window (runahead_ns; with use_dynamic_runahead, the longest
 * route latency if that is more), because the last window of such a run starts below T and may
 * end that much past it — a datagram submitted later would find its window gone (send_time
 * below the window start: SGN_EINVAL). When the simulation has run dry, or the next send lies
 * before the device's next event, sgn_set_window moves the window to it as before.
 * Shards: a datagram goes to the shard that owns src_host (anything else is SGN_EINVAL). Each
 * shard numbers its own submissions, so the slot bits of a drain record's tag (tag &
 * SGN_TAG_SLOT_MASK) are per submitting shard, and the record carries the submitted handle
 * only where the shard that drains it also submitted it: fates decided at the source (LOCAL,
 * LOSS, UNKNOWN, BLOCKED) always do; DELIVERED and CODEL records, which appear at the
 * destination, carry handle 0 when the destination belongs to another shard (src_host and
 * src_eid identify the datagram there). */
typedef struct sgn_pkt_soa {
  uint64_t n;
  const uint32_t* src_host;    /* [n] HostId */
  const uint32_t* dst_ip;      /* [n] IPv4, host byte order (unknown: InetDropped) */
  const uint32_t* payload_len; /* [n] UDP payload bytes */
  const uint32_t* wire_len;    /* [n] or NULL */
  const uint64_t* send_time;   /* [n] EmulatedTime */
  const uint64_t* handle;      /* [n] opaque, returned by sgn_drain (may be NULL: 0) */
} sgn_pkt_soa;
int sgn_submit(sgn_ctx* ctx, const sgn_pkt_soa* batch);

/* Per-thread staging: Shadow calls Worker::send_packet from every worker thread
 * at once (router/mod.rs:70-73, worker.rs:330). Each CPU worker thread owns one stage and
 * appends to it with sgn_stage_push — safe concurrently on DISTINCT stages, no device work;
 * the controller thread then submits every stage with one sgn_stage_flush between rounds.
 * A flush is exactly one sgn_submit of the stages' datagrams concatenated in stage-creation
 * order (each stage in push order); on failure nothing is queued and the stages keep their
 * datagrams. A push that runs while a flush runs is either part of that flush or stays
 * staged for the next one (a flush clears only what it copied). Create and destroy stages
 * only while no flush runs. */
typedef struct sgn_stage sgn_stage;
int sgn_stage_create(sgn_ctx* ctx, sgn_stage** out);
void sgn_stage_destroy(sgn_stage* stage);
/* Copies the batch into the stage (checks array presence and payload/wire sizes only; the
 * window and horizon rules are checked at flush). */
int sgn_stage_push(sgn_stage* stage, const sgn_pkt_soa* batch);
/* Datagrams waiting in a stage. */
uint64_t sgn_stage_pending(const sgn_stage* stage);
int sgn_stage_flush(sgn_ctx* ctx);

/* Packet egress: one record per datagram that left the network core, on the host where it
 * happened. Every submitted datagram yields exactly one record (delivered or dropped) once
 * its fate is decided; datagrams sent to EXTERNAL hosts are all submitted ones. */
#define SGN_DRAIN_DELIVERED 0u /* handed to the destination's interface (relay_inet_in) */
#define SGN_DRAIN_LOCAL 1u     /* to the host's own address (loopback, relay is_local) */
#define SGN_DRAIN_LOSS 2u      /* dropped by path reliability at send (worker.rs:366-371) */
#define SGN_DRAIN_UNKNOWN 3u   /* destination not in the simulation (InetDropped, :347) */
#define SGN_DRAIN_CODEL 4u     /* dropped by the destination router's CoDel (:319-321) */
#define SGN_DRAIN_BLOCKED 5u   /* the source's socket send queue was full */
typedef struct sgn_drain_rec {
  uint64_t time;        /* when it happened (EmulatedTime) */
  uint64_t src_eid;     /* source event id (DELIVERED / CODEL; 0 otherwise) */
  uint64_t handle;      /* sgn_submit handle (0 if submitted on another shard) */
  uint32_t host;        /* HostId where it happened */
  uint32_t src_host;    /* sender HostId */
  uint32_t dst_host;    /* destination HostId (0xFFFFFFFF unknown / not resolved) */
  uint32_t status;      /* SGN_DRAIN_* */
  uint32_t payload_len;
  uint32_t tag;         /* SGN_TAG_EXT | header kind << 29 | submission slot (sgn_workload.h) */
} sgn_drain_rec;
/* Device buffer for drain records between two sgn_drain calls (before sgn_sim_init;
 * default 1<<20 for EXTERNAL traffic). Running out is SGN_EOVERFLOW at the round. */
int sgn_drain_enable(sgn_ctx* ctx, uint64_t capacity);
/* Moves the records of hosts [host_lo, host_hi) out, ordered by (host, time, src_host,
 * src_eid, tag, status); records of other hosts stay for a later call. At most cap are
 * returned (*n_out); the rest stay. Between rounds only. */
int sgn_drain(sgn_ctx* ctx, uint32_t host_lo, uint32_t host_hi, sgn_drain_rec* out, uint64_t cap,
              uint64_t* n_out);

/* ---- additions to ABI 10 (new calls only; no struct of ABI 10 changes): the ordered drain —
 * every pending record in one call, ordered on the device, with per-host spans, all or nothing
 * (the form of sgn_trace_take; sgn_drain above stays the range form). DESIGN.md §7f. ---- */

/* Drain records produced and not yet returned: those on the device plus those an earlier
 * sgn_drain left held on the host (another host range, a short cap). */
int sgn_drain_pending(sgn_ctx* ctx, uint64_t* n);

/* Between rounds: moves EVERY pending record out, ordered on the device by sgn_drain's key
 * (host, time, src_host, src_eid, tag, status), with one span per host that has records
 * (ascending HostId; sgn_trace_span: out[first .. first + count)). The result is byte for byte
 * what sgn_drain(ctx, 0, 0xFFFFFFFF, out, enough, &n) would return at that point, handle included
 * (the shard rule above), and the context is left as that call would leave it: nothing on the
 * device, nothing held. Records an earlier sgn_drain left held are part of the take.
 * All or nothing: with cap below the pending count, or spans != NULL and span_cap below the
 * hosts with records, SGN_ERANGE, *n_out and *n_spans say what is needed, and nothing is taken or
 * changed; the same call with larger arrays then succeeds. spans may be NULL with span_cap 0.
 * With nothing pending: SGN_OK, both counts 0, nothing is launched.
 * The simulation does not change (window, counters, digests, traces, sampler and backlog are
 * those of a run with sgn_drain in its place); snapshots save and restore pending records as
 * they do for sgn_drain. Works on any context and is not a collective: a shard takes the records
 * of the hosts it owns. A record whose host lies outside the owned range is SGN_EDEVICE (the
 * message names the host) with nothing taken.
 * Errors: SGN_EINVAL for a null ctx or n_out, or a null array with a non-zero capacity;
 * SGN_ESTATE without a simulation or with traffic other than EXTERNAL; SGN_ENOMEM with nothing
 * changed; SGN_EDEVICE for a HIP failure. */
int sgn_drain_take(sgn_ctx* ctx, sgn_drain_rec* out, uint64_t cap, uint64_t* n_out,
                   sgn_trace_span* spans, uint64_t span_cap, uint64_t* n_spans);

/* What the context's last sgn_drain_take (or sgn_selftest_drain_order) spent (measurements;
 * tools/drain_timing.py). wave_max and tile are always filled. */
typedef struct sgn_drain_take_timing {
  double total_ms, kernel_ms[4] /* count, scan, scatter, order */, copy_ms;
  uint64_t records, hosts, largest_span;
  uint64_t spans_by_class[3];   /* ordered by a wave / by one workgroup in LDS / by tiles + merge */
  uint32_t wave_max, tile;      /* the class limits: records a wave, and a workgroup, orders at once */
} sgn_drain_take_timing;
int sgn_drain_take_timing_get(sgn_ctx* ctx, sgn_drain_take_timing* out);

/* ---- additions to ABI 10 (new calls only; no struct of ABI 10 changes): the router delay report —
 * how long every packet spent at its destination's router (the CoDel queue, then the wait for the
 * downlink token bucket) before it was handed to the interface or dropped, folded on the device
 * from the trace. The ROUTER DELAY of a packet at host h is the `a` of its exit record
 * (SGN_TRACE_DELIVER or SGN_TRACE_CODEL_DROP) minus the `a` of its SGN_TRACE_POP record; loopback
 * (SGN_TRACE_LOCAL) packets never enter the router and are not counted. Within one host the router
 * is FIFO, so the k-th exit of a host pairs with its k-th POP: the report ranks the pops and the
 * exits inside the per-host spans a take already builds and matches them there; no record leaves
 * the device. Packets in the router when an interval ends carry over to the next fold (the CARRY:
 * per owned host the FIFO of packets popped and not yet exited — pop time, source host, source
 * event id — in device memory, grown on demand). DESIGN.md §7g.
 * Histogram bins: bin 0 holds delay == 0, bin k (1 <= k <= 46) holds 2^(k-1) <= delay < 2^k ns,
 * bin 47 everything from 2^46 ns up. ---- */

#define SGN_DELAY_BINS 48
typedef struct sgn_delay_row {      /* 64 B: one per owned host with anything to report */
  uint32_t host, reserved;
  uint32_t standing;                /* carry length now: packets popped into the router and not yet exited */
  uint32_t unmatched;               /* exits that met an unknown entry (a packet that stood there at sgn_delay_enable) */
  uint64_t delivered, dropped;      /* matched exits by kind (DELIVER / CODEL_DROP) */
  uint64_t delay_sum_delivered, delay_sum_dropped;   /* ns */
  uint64_t delay_max;               /* over both kinds */
  uint64_t standing_oldest;         /* pop time of the carry's head; SGN_EMUTIME_INVALID when empty or unknown */
} sgn_delay_row;
typedef struct sgn_delay_info {
  uint64_t rounds, window_start, window_end;   /* the round edge of the last fold (sgn_window) */
  uint64_t folds, records;                     /* folds, and trace records folded, since enable / clear */
  uint64_t hosts, rows;                        /* owned hosts; hosts with a row */
  uint64_t total[6];   /* delivered, dropped, delay_sum_delivered, delay_sum_dropped, standing, unmatched */
  uint64_t delay_max;  uint32_t delay_max_host, pad0;   /* over the hosts with a matched exit: lowest HostId on
                                                           equal values; 0 / 0 when none */
  uint64_t hist_delivered[SGN_DELAY_BINS], hist_dropped[SGN_DELAY_BINS];
} sgn_delay_info;

/* After sgn_sim_init on a context with a trace, between calls. SGN_ESTATE without a simulation,
 * without a trace, or with trace records pending (sgn_trace_take them first: the record stream and
 * the device state then meet at one round edge). Zeroes the accumulators and seeds each owned
 * host's carry with as many UNKNOWN entries (pop time SGN_EMUTIME_INVALID) as packets stand at its
 * router now: the CoDel queue's length plus the packet relay_inet_in holds (sgn_backlog's
 * router_packets and SGN_BACKLOG_ROUTER_HELD, by the same reader). Right after sgn_sim_init that
 * is nothing. An exit that meets an unknown entry counts as `unmatched` and enters no statistic.
 * May be called again at any time (the report starts over from the state as it is now).
 * SGN_ENOMEM leaves the context without the report. */
int sgn_delay_enable(sgn_ctx* ctx);

/* Between calls: a take whose records stay on the device. Orders every pending trace record as
 * sgn_trace_take does (the same kernels and checks), folds them into the report and empties the
 * trace buffer. With nothing pending: SGN_OK, only `folds` advances. All or nothing: on any error
 * nothing is consumed, accumulators and carry are unchanged. SGN_EDEVICE, naming the first host,
 * when a host has more exits than carry plus pops, when an exit comes before its pop, or when a
 * matched pair disagrees in (peer, c) or has its exit time before its pop time. out (may be NULL)
 * gets the info sgn_delay_get would return.
 * On a context with the report enabled sgn_trace_take folds the same ordered records before it
 * copies them out; its output bytes, spans and counts are what they are without the report, so
 * captures and the report work together (the two calls share one function).
 * Rewinds: the report remembers the trace position it has folded up to. When a fold or take finds
 * the context's taken count different from it (sgn_snapshot_restore moved it back), SGN_ESTATE and
 * nothing changes, until sgn_delay_enable is called again. The report is not part of a snapshot
 * or a snapshot file.
 * Works on any context for the hosts it owns and is not a collective (pop and exit both happen at
 * the destination). With sgn_trace_hosts only the listed hosts produce records and rows. */
int sgn_delay_fold(sgn_ctx* ctx, sgn_delay_info* out /* may be NULL */);

/* Rows for every owned host with a non-zero standing, unmatched, delivered or dropped, ascending
 * by HostId, compacted on the device (count, scan, scatter); totals, maxima and both histograms
 * are folded on the device. out == NULL with cap == 0 asks for the totals only; with out != NULL
 * and cap below the row count SGN_ERANGE, *n_out says what is needed, info is filled and nothing
 * is written to out (sgn_backlog's rules). Read-only, cumulative since the last enable or clear.
 * Errors: null ctx, n_out or info SGN_EINVAL; report not enabled SGN_ESTATE. */
int sgn_delay_get(sgn_ctx* ctx, sgn_delay_row* out, uint64_t cap, uint64_t* n_out, sgn_delay_info* info);

/* Zeroes the accumulators, both histograms, folds and records. The carry stays, so a caller makes
 * intervals with get + clear and loses no match. */
int sgn_delay_clear(sgn_ctx* ctx);

/* What the context's last fold spent (sgn_delay_fold, sgn_trace_take with the report enabled, or
 * sgn_selftest_delay_fold's last piece; tools/delay_timing.py). wave_max and tile are always
 * filled. */
typedef struct sgn_delay_timing {
  double total_ms;       /* wall time of the call */
  double order_ms[3];    /* the take's kernels: count, scan, scatter */
  double kernel_ms[5];   /* per-host pop / exit counts; carry scan; carry survivors; rank and match; commit */
  uint64_t records, hosts, largest_span, carry_entries;
  uint64_t spans_by_class[2];   /* matched by a wave / walked by a workgroup */
  uint32_t wave_max, tile;      /* the class limits: records a wave, and a workgroup per pass, handle at once */
} sgn_delay_timing;
int sgn_delay_timing_get(sgn_ctx* ctx, sgn_delay_timing* out);

/* The next window, decided by a caller that also runs hosts of its own (Controller with CPU
 * hosts, controller.rs:88-112): [start, end) with previous window end <= start <= the
 * device's minimum next event time (sgn_window's start), start < end, end - start <= the
 * runahead the calendar was sized for, end clamped to the stop time. */
int sgn_set_window(sgn_ctx* ctx, uint64_t start, uint64_t end);

/* The host RNG, held on the device (the one authoritative copy): CPU-side draws
 * of host_rngDouble / host_rngNextNBytes (host/host.rs:1324-1336) and raw next_u64. They
 * advance the same Xoshiro256++ stream the loss draws use. Between rounds only. */
int sgn_rng_next_u64(sgn_ctx* ctx, uint32_t host, uint64_t* out);
/* counts[i] draws from each of n DISTINCT owned hosts in one device pass, concatenated in
 * order into out (sum(counts) entries): the batched form of sgn_rng_next_u64. */
int sgn_rng_next_u64_batch(sgn_ctx* ctx, const uint32_t* hosts, const uint32_t* counts, uint32_t n,
                           uint64_t* out);
/* rand 0.9 StandardUniform f64: (next_u64 >> 11) * 2^-53 */
int sgn_rng_double(sgn_ctx* ctx, uint32_t host, double* out);
/* rand_core 0.9 fill_bytes_via_next: little-endian next_u64 per 8 bytes; a tail of 5..7
 * bytes takes the low bytes of one more next_u64, a tail of 1..4 those of next_u32 (the
 * upper half of next_u64, rand_xoshiro 0.7). */
int sgn_rng_fill_bytes(sgn_ctx* ctx, uint32_t host, uint8_t* buf, size_t len);

/* Engine layout and execution mode chosen by sgn_sim_init (capacity planning, tests). */
typedef struct sgn_engine_info {
  uint64_t calendar_buckets;    /* NB: time buckets of the event calendar (a power of two) */
  uint64_t bucket_width_ns;     /* BW = max(min route latency, configured runahead) */
  uint64_t host_groups;         /* G: groups of hosts_per_wave consecutive hosts */
  uint64_t slab_capacity;       /* event runs per (bucket, group) slab */
  uint64_t hosts_per_wave;
  uint64_t persistent_grid;     /* workgroups of the persistent round kernel (0: per-round) */
  uint64_t persistent_fallbacks;/* persistent launches refused by the residency census */
  uint64_t device_bytes;        /* device memory held by the simulation */
  /* multi-shard round exchange (0 on one shard): per-peer slot capacity, runs per peer the
   * current rounds' send/recv move (sized from the high-water mark; a round that needs more
   * is held and completed with a full-slot exchange), the largest per-peer run count of any
   * round so far, rounds completed that way, and bytes sent to peers since sim_init */
  uint64_t exchange_slot_runs;
  uint64_t exchange_send_runs;
  uint64_t exchange_hwm_runs;
  uint64_t exchange_spills;
  uint64_t exchange_bytes;
  /* CoDel queues: pages of 16 runs in the shared pool (codel_cap slots per host on average,
   * at least one page per host), and pages taken from its free ring so far */
  uint64_t codel_pages;
  uint64_t codel_page_allocs;
  uint64_t codel_pages_free;     /* pages in the free ring now */
  uint64_t codel_pages_chained;  /* pages in the hosts' queue chains now (read from the host
                                    records: free + chained == codel_pages, no page lost) */
  uint64_t compute_units;        /* of this context's GPU */
  uint64_t bucket_min_lds;       /* 1: round kernels fold bucket minima in LDS first */
  /* ABI 7: device pools grow instead of refusing a scenario (the reference's queues are
   * unbounded, codel_queue.rs:33,303-317, event_queue.rs:57-66). A round that could need more
   * than a pool holds is held at its start (nothing of it has run), the pool grows between
   * launches, and the round runs. */
  uint64_t lds_per_cu;           /* LDS bytes per CU the residency model used (device attribute) */
  uint64_t codel_pool_grows;     /* CoDel page pool enlargements */
  uint64_t calendar_grows;       /* calendar re-layouts with larger slabs */
  uint64_t calendar_spill_runs;  /* runs that went to the calendar's spill area (then re-filed) */
  uint64_t exchange_slot_grows;  /* multi-shard exchange slot enlargements */
  uint64_t rounds_held;          /* rounds held at their start for a pool to grow */
  /* ABI 8: hot slabs. A (bucket, host group) slab past its capacity continues in an extension
   * (laid out at a held round edge); a slab holding more runs than one workgroup's LDS orders
   * at once is ordered and executed in pieces in Shadow's key order (event.rs:84-155), so no
   * fan-in is refused (the reference's EventQueue is an unbounded BinaryHeap,
   * core/work/event_queue.rs:12,57-66). */
  uint64_t slab_extensions;      /* slabs with an extension now */
  uint64_t slab_extension_runs;  /* runs the extensions hold in total */
  uint64_t big_slab_pieces;      /* pieces run by the big-slab path since sim_init */
  uint64_t spill_area_runs;      /* the spill area's capacity */
  uint64_t spill_area_grows;     /* spill area enlargements */
  /* ABI 9: persistent multi-shard rounds. With N > 1 shards the rounds run in one persistent
   * launch per GPU (or, for a local group on one GPU, one launch whose workgroup ranges are the
   * shards): runs for another shard go straight into that shard's inbox (peer-mapped memory),
   * and every shard computes the next window from the N round-edge messages in its inbox
   * (core/manager.rs:568-628, core/controller.rs:88-112). */
  uint64_t exchange_mode;        /* 0: one shard; 1: per-round launches + RCCL send/recv (or the
                                    local group's copies); 2: persistent rounds, peer inboxes */
  uint64_t inbox_slot_runs;      /* runs per sender and round parity in each inbox */
  uint64_t inbox_grows;          /* inbox enlargements (a round used more than half a slot) */
  uint64_t inbox_overflow_rounds;/* rounds whose runs past a slot the host moved */
  uint64_t inbox_moved_runs;     /* ... runs moved that way (into this shard) */
  uint64_t persistent_x_launches;/* persistent multi-shard launches */
  uint64_t persistent_x_grid;    /* this shard's workgroups in the last one */
} sgn_engine_info;
int sgn_engine_info_get(sgn_ctx* ctx, sgn_engine_info* out);

/* Device timing of the engine's kernels since sim_init (needs SGN_CREATE_TIME_KERNELS or
 * SGN_CREATE_TIME_EXECUTE). Persistent launches (k_rounds, many rounds each) are all timed;
 * per-round launches are timed one in eight (an event pair around every launch cost ~20 % of
 * the rounds), so launches[k] / ms[k] cover that sample: the average duration is
 * ms[k] / launches[k], and launches_total[k] counts every launch (timed or not) to scale
 * it to the total. */
typedef struct sgn_kernel_times {
  uint64_t launches[16];         /* timed launches */
  double ms[16];                 /* their summed duration */
  const char* name[16];
  uint32_t n_kernels;
  uint64_t launches_total[16];   /* every launch since sim_init (ABI 7) */
} sgn_kernel_times;
int sgn_kernel_times_get(sgn_ctx* ctx, sgn_kernel_times* out);

/* ------------------------------------------------------------------------------------ */
/* Multi-GPU shard exchange (round edge). Hosts are partitioned into contiguous HostId   */
/* ranges; events for remote hosts leave through per-peer slots and the window minimum */
/* is reduced across shards. The library drives RCCL itself on its own stream.         */
/* ------------------------------------------------------------------------------------ */

/* Size of the opaque RCCL unique id blob (ncclUniqueId). */
#define SGN_COMM_ID_BYTES 128
/* Rank 0 produces the id; the caller broadcasts it (e.g. torch.distributed) to all ranks. */
int sgn_comm_get_unique_id(uint8_t id_out[SGN_COMM_ID_BYTES]);
/* Creates the communicator over shard_count ranks; this ctx is rank shard_rank.
 * exchange_slot_events = capacity (events) of each per-peer slot per round. */
int sgn_comm_init(sgn_ctx* ctx, const uint8_t id[SGN_COMM_ID_BYTES],
                  uint64_t exchange_slot_events);
/* Local shard group: ctxs[i] is shard i of n (sgn_create with shard_count n) in THIS
 * process, on any devices (several may share one GPU). The round edge runs with device
 * copies instead of RCCL (host-synchronous per round): a test transport that exercises the
 * same device-side multi-shard path. Call before sgn_sim_init on every context; drive the
 * rounds with sgn_run_local_group (not sgn_run). */
int sgn_comm_init_local(sgn_ctx* const* ctxs, uint32_t n, uint64_t exchange_slot_events);
int sgn_run_local_group(sgn_ctx* const* ctxs, uint32_t n, uint64_t max_rounds,
                        uint64_t* rounds_done);
/* Owned HostId range of a shard (same split on every rank). */
int sgn_shard_range(uint32_t n_hosts, uint32_t shard_rank, uint32_t shard_count,
                    uint32_t* host_lo, uint32_t* host_hi);

/* ------------------------------------------------------------------------------------ */
/* CPU-side consumers (core/worker.rs:657-690, host/host.rs:1325-1336)                  */
/* ------------------------------------------------------------------------------------ */

/* worker_getLatency (worker.rs:657-667): addresses in NETWORK byte order; returns
 * SimulationTime ns or SGN_EMUTIME_INVALID (= SIMTIME_INVALID) if either is unknown. */
uint64_t sgn_worker_get_latency(sgn_ctx* ctx, uint32_t src_be, uint32_t dst_be);
/* worker_isRoutable (worker.rs:684-690). */
int32_t sgn_worker_is_routable(sgn_ctx* ctx, uint32_t src_be, uint32_t dst_be);
/* worker_getBandwidth{Up,Down}Bytes (worker.rs:670-681): bits / 8; 0 if unknown. */
uint64_t sgn_worker_get_bandwidth_up_bytes(sgn_ctx* ctx, uint32_t ip_be);
uint64_t sgn_worker_get_bandwidth_down_bytes(sgn_ctx* ctx, uint32_t ip_be);
/* Dns::addr_to_host_id (network/dns.rs:174): 0 and *host set, or SGN_ENOENT. */
int sgn_addr_to_host_id(sgn_ctx* ctx, uint32_t ip, uint32_t* host);

/* ------------------------------------------------------------------------------------ */
/* Front end (drop-in graph ingest): GML text -> sgn_graph (lib/gml-parser, graph/mod.rs)*/
/* ------------------------------------------------------------------------------------ */

typedef struct sgn_gml sgn_gml;
/* Parses GML text as gml_parser::parse + NetworkGraph::parse do (lib/gml-parser/src/
 * parser.rs:66-230, network/graph/mod.rs:28-179, units.rs:406-440). On failure returns
 * SGN_EINVAL and, if err/err_len given, a message. */
int sgn_gml_parse(const char* text, size_t len, sgn_gml** out, char* err, size_t err_len);
void sgn_gml_free(sgn_gml* g);
/* Borrowed view valid until sgn_gml_free. */
int sgn_gml_graph(const sgn_gml* g, sgn_graph* out);
/* Node bandwidths from host_bandwidth_up/_down (bits/s); has_* = 0 when absent. */
int sgn_gml_node_bandwidth(const sgn_gml* g, uint32_t node_index, uint64_t* up_bits,
                           int32_t* has_up, uint64_t* down_bits, int32_t* has_down);

/* assign_ips (core/sim_config.rs:386-407) over IpAssignment (network/graph/mod.rs:355-417),
 * hosts in HostId (= hostname) order. Hosts with explicit_ip[i] != 0 keep ips[i] (host byte
 * order) and are registered first; a repeated configured address is SGN_EINVAL with
 * *bad_host = the later host. Every other host gets the next address after the last one
 * handed out (from 11.0.0.0), skipping x.x.x.0, x.x.x.255 and configured addresses;
 * SGN_ERANGE past 255.255.255.254. Host-side only. */
int sgn_assign_ips(uint32_t n, const uint8_t* explicit_ip, uint32_t* ips, uint32_t* bad_host);

/* units.rs:406-440 FromStr + convert(): parse "10 ms" / "81920 Kibit" / "1 GiB".
 * kind: 0 Time -> ns, 1 Bytes -> bytes, 2 BitsPerSec -> bits/s. */
int sgn_units_parse(int32_t kind, const char* text, uint64_t* value_base);

/* ------------------------------------------------------------------------------------ */
/* Packet capture (utility/pcap_writer.rs, network/packet.rs:800-934, interface.rs:192-215)  */
/* ------------------------------------------------------------------------------------ */

typedef struct sgn_pcap sgn_pcap;
/* PcapWriter::new: a file with the libpcap global header (magic 0xA1B2C3D4, v2.4, zone 0,
 * sigfigs 0, snaplen = capture_len, link type 101 raw IP), native byte order. */
int sgn_pcap_open(const char* path, uint32_t capture_len, sgn_pcap** out);
/* PcapWriter::write_packet: record header {ts_sec, ts_usec, min(len, capture_len), len}
 * and the first min(len, capture_len) bytes. */
int sgn_pcap_write_packet(sgn_pcap* p, uint32_t ts_sec, uint32_t ts_usec, const uint8_t* bytes,
                          uint32_t len);
int sgn_pcap_close(sgn_pcap* p);
/* Packet::display_bytes for the path's packets: the IPv4 header (0x45, DSCP 0, total length,
 * id 0, DF, TTL 64, protocol, checksum 0, addresses), then a UDP header (ports, length,
 * checksum 0) or, by the tag's header kind, a TCP header (20 B, or 24 B with the window
 * scale option 3,3,ws + padding), then the payload. The synthetic applications have no
 * sockets: ports, TCP sequence/ack/flags/window and the payload bytes are 0. Returns the
 * packet length (header + payload) and writes min(that, cap) bytes. */
uint32_t sgn_packet_bytes(uint32_t src_ip, uint32_t dst_ip, uint32_t payload_len, uint32_t tag,
                          uint8_t* out, uint32_t cap);
/* One host's interface capture from trace records (any order; the host's records are taken
 * in seq order): every IF_POP record (send side) and every DELIVER and LOCAL record
 * (receive side) is one captured packet, stamped with the record's time as
 * to_abs_simtime (seconds saturated to u32, microseconds). host_ip[HostId] gives addresses;
 * an unknown peer's address is the record's c. Returns the number of packets written. */
int64_t sgn_trace_pcap(const sgn_trace_rec* recs, uint64_t n, uint32_t host, const uint32_t* host_ip,
                       uint32_t n_hosts, const char* path, uint32_t capture_len);
/* (addition to ABI 10) The same packets appended to an open writer, with the writer's capture
 * length: sgn_trace_pcap is sgn_pcap_open + this + sgn_pcap_close. A capture written piece by
 * piece (one call per sgn_trace_take, the pieces in the order they were taken) has the bytes of
 * one written from the whole trace. Returns the packets written, SGN_EINVAL for a null argument
 * or a peer outside [0, n_hosts). */
int64_t sgn_pcap_write_trace(sgn_pcap* p, const sgn_trace_rec* recs, uint64_t n, uint32_t host,
                             const uint32_t* host_ip, uint32_t n_hosts);

/* ------------------------------------------------------------------------------------ */
/* Test hooks (not part of the reference interface)                                      */
/* ------------------------------------------------------------------------------------ */

/* Device CoDel control-law increments round(1e8 / sqrt(count)) for count in [0, n)
 * (router/codel_queue.rs:285-298), for checking device f64 rounding against the host. */
int sgn_selftest_codel_law(sgn_ctx* ctx, uint64_t n, uint64_t* out);

/* The reports' exclusive scan (sgn_sample's scan kernel itself, one workgroup walking the counts in
 * tiles of 1024) on the caller's n counts: off_out[j] = counts[0] + ... + counts[j - 1], *total_out
 * their sum. Needs no simulation; for checking the carry from tile to tile. */
int sgn_selftest_report_scan(sgn_ctx* ctx, const uint32_t* counts, uint32_t n, uint32_t* off_out, uint64_t* total_out);

/* sgn_drain_take's kernels (count, scan, scatter, order) on the caller's n records of hosts
 * [host_lo, host_lo + n_hosts): out gets them ordered by (host, time, src_host, src_eid, tag,
 * status), spans (may be NULL with span_cap 0) one entry per host with records; span_cap below
 * that count is SGN_ERANGE with *n_spans the count. Needs no simulation; handle is copied through
 * untouched. Records with equal keys come out in an unspecified order. A record of a host outside
 * the range is SGN_EDEVICE with out untouched. */
int sgn_selftest_drain_order(sgn_ctx* ctx, const sgn_drain_rec* recs, uint64_t n, uint32_t host_lo,
                             uint32_t n_hosts, sgn_drain_rec* out, sgn_trace_span* spans,
                             uint64_t span_cap, uint64_t* n_spans);

/* The router delay report's kernels (the take's ordering, then count, scan, carry, rank and match,
 * commit, and sgn_delay_get's compaction) without a simulation: the caller's records of hosts
 * [host_lo, host_lo + n_hosts), in any order, are n_pieces consecutive intervals, piece i being
 * recs[piece_ends[i - 1] .. piece_ends[i]) (piece_ends ascending; every host's records of a piece
 * carry consecutive seq). The carry starts from standing0[h] unknown entries per host (NULL: none).
 * rows / cap / n_rows / info as sgn_delay_get after the last piece. An enabled report of the
 * context is left alone. */
int sgn_selftest_delay_fold(sgn_ctx* ctx, const sgn_trace_rec* recs, const uint64_t* piece_ends, uint32_t n_pieces,
                            uint32_t host_lo, uint32_t n_hosts, const uint32_t* standing0 /* may be NULL */,
                            sgn_delay_row* rows, uint64_t cap, uint64_t* n_rows, sgn_delay_info* info);

/* The section digest of snapshot files, for len % 4 == 0: with w_j the little-endian u64 at byte
 * 8j (a 4-byte tail zero-extended), D = mix64(len ^ SGN_DIGEST_SEED) + sum_j mix64(w_j ^
 * (0x9e3779b97f4a7c15 * (j + 1))) mod 2^64 (sgn_mix64, sgn_workload.h): position-keyed terms under
 * a commutative sum, so any order of evaluation gives the same value. sgn_digest_bytes is the host
 * form (0 for len % 4 != 0 or a null p with len > 0); sgn_selftest_digest runs the device kernel
 * on a copy of host_bytes. */
uint64_t sgn_digest_bytes(const void* p, size_t len);
int sgn_selftest_digest(sgn_ctx* ctx, const void* host_bytes, size_t len, uint64_t* out);

/* What the context's last sgn_snapshot_export / _import spent (measurements; tools/snapshot_timing.py). */
typedef struct sgn_snapshot_file_timing {
  double total_ms;       /* wall time of the call */
  double stream_ms;      /* ... of which the payloads: device <-> pinned chunk <-> callback */
  double digest_ms;      /* HIP-event time of the one digest launch over the device sections */
  uint64_t device_bytes; /* bytes that launch read */
  uint64_t file_bytes;
} sgn_snapshot_file_timing;
int sgn_snapshot_file_timing_get(sgn_ctx* ctx, sgn_snapshot_file_timing* out);

/* Diagnostics of the last execute launch, SGN_STAMP_WORDS u64 per wave: {shader cycles,
 * events handled, max events of one host, hosts with events, then (diagnostic build
 * libsgn_diag.so only) lane 0's per-event-kind cycles and counts}. Needs SGN_STAMPS=1 in
 * the environment at sgn_sim_init; n = number of waves (0 when disabled), cap in waves. */
#define SGN_STAMP_WORDS 96
int sgn_debug_stamps(sgn_ctx* ctx, uint64_t* out, uint64_t cap, uint64_t* n);
/* Per-round timeline of the last persistent launch (SGN_STAMPS=1): 128 x {earliest round
 * start, latest arrival at the round barrier, round edge done} on the 100 MHz clock. */
int sgn_debug_rounds(sgn_ctx* ctx, uint64_t* out);
/* the persistent multi-shard kernel's per-round timeline (SGN_STAMPS=2): 8 words per round for 128
 * rounds — earliest start, latest local arrival, local barrier seen, messages sent, latest "all
 * messages seen", latest imports filed, latest second barrier seen (100 MHz clock); resets */
int sgn_debug_rounds_x(sgn_ctx* ctx, uint64_t* out);
/* the same per workgroup (SGN_STAMPS=3: plain stores, no shared words): [128 rounds][2048
 * workgroups of this shard][8] u64, the same 8 stamps (0: not written); resets */
int sgn_debug_rounds_xw(sgn_ctx* ctx, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* SGN_H */
