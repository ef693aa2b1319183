"""ctypes binding of libsgn (include/sgn.h) plus the synthetic-workload generators.

This module is host-side plumbing for tests and bench.py: every computation of the packet
core happens inside libsgn.so on the GPU. Loading fails loudly if the library is missing;
there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
# SGN_LIB overrides the library file (diagnostic builds such as libsgn_diag.so)
LIB_PATH = pathlib.Path(os.environ["SGN_LIB"]) if os.environ.get("SGN_LIB") else HERE / "libsgn.so"

SIMULATION_START = 946684800 * 1_000_000_000
EMUTIME_INVALID = 0xFFFFFFFFFFFFFFFF
EMUTIME_MAX = 0xFFFFFFFFFFFFFFFE
TRAFFIC_PERIODIC = 1
TRAFFIC_TGEN = 2
TRAFFIC_EXTERNAL = 3  # CPU-resident apps: sgn_submit / sgn_drain
QDISC_FIFO, QDISC_ROUND_ROBIN = 0, 1
TAG_EXT = 0x80000000
DRAIN_DELIVERED, DRAIN_LOCAL, DRAIN_LOSS, DRAIN_UNKNOWN, DRAIN_CODEL, DRAIN_BLOCKED = range(6)
STAMP_WORDS = 96  # include/sgn.h SGN_STAMP_WORDS
CREATE_TIME_KERNELS = 1

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f32p = C.POINTER(C.c_float)


class Graph(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_uint32),
        ("node_id", u32p),
        ("n_edges", C.c_uint32),
        ("edge_src", u32p),
        ("edge_dst", u32p),
        ("edge_latency_ns", u64p),
        ("edge_loss", f32p),
        ("directed", C.c_int32),
    ]


class Hosts(C.Structure):
    _fields_ = [
        ("n_hosts", C.c_uint32),
        ("ip", u32p),
        ("node_id", u32p),
        ("bw_up_bits", u64p),
        ("bw_down_bits", u64p),
        ("seed", u64p),
    ]


class SimConfig(C.Structure):
    _fields_ = [
        ("stop_time_ns", C.c_uint64),
        ("bootstrap_end_ns", C.c_uint64),
        ("runahead_ns", C.c_uint64),
        ("use_dynamic_runahead", C.c_int32),
        ("out_fifo_cap", C.c_uint32),
        ("codel_cap", C.c_uint32),
        ("hosts_per_wave", C.c_uint32),
        ("event_capacity", C.c_uint64),
        ("interface_qdisc", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class Traffic(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("payload_len", C.c_uint32),
        ("flow_seed", C.c_uint64),
        ("start_ns", C.c_uint64),
        ("start_jitter_ns", C.c_uint64),
        ("period_ns", C.c_uint64),
        ("period_jitter_ns", C.c_uint64),
        ("unknown_dst_permille", C.c_uint32),
        ("req_payload", C.c_uint32),
        ("n_servers", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("server_hosts", u32p),
        ("file_bytes", C.c_uint64 * 3),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rounds", "packets_sent", "packets_loss_dropped", "packets_unknown_dst",
        "packet_events_popped", "codel_dropped", "delivered", "local_delivered",
        "app_blocked", "local_events", "bytes_delivered", "min_used_latency_ns",
        "max_codel_len", "max_pending_events", "host_executions",
        "sched_heavy_hosts", "sched_sorted_segments", "event_runs")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class HostDigest(C.Structure):
    _fields_ = [
        ("tx", C.c_uint64), ("rx", C.c_uint64), ("app", C.c_uint64),
        ("rng", C.c_uint64 * 4), ("next_event_id", C.c_uint64),
        ("n_sent", C.c_uint64), ("n_popped", C.c_uint64), ("n_delivered", C.c_uint64),
        ("n_codel_dropped", C.c_uint64),
    ]


class TraceRec(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32), ("host", C.c_uint32), ("peer", C.c_uint32), ("flags", C.c_uint32),
        ("a", C.c_uint64), ("b", C.c_uint64), ("c", C.c_uint64), ("seq", C.c_uint64),
        ("rng_pos", C.c_uint64),
    ]


TRACE_DTYPE = np.dtype([("kind", "<u4"), ("host", "<u4"), ("peer", "<u4"), ("flags", "<u4"),
                        ("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("seq", "<u8"), ("rng_pos", "<u8")])
TRACE_SEND, TRACE_POP, TRACE_DELIVER, TRACE_CODEL_DROP, TRACE_IF_POP, TRACE_LOCAL = 1, 2, 3, 4, 5, 6
class TraceSpan(C.Structure):
    _fields_ = [("host", C.c_uint32), ("reserved", C.c_uint32), ("first", C.c_uint64), ("count", C.c_uint64)]


SPAN_DTYPE = np.dtype([("host", "<u4"), ("reserved", "<u4"), ("first", "<u8"), ("count", "<u8")])
assert SPAN_DTYPE.itemsize == C.sizeof(TraceSpan)
ERANGE = -34


class TraceTakeTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("kernel_ms", C.c_double * 3), ("copy_ms", C.c_double),
                ("records", C.c_uint64), ("hosts", C.c_uint64)]


SAMPLE_FIELDS = ("sent", "popped", "delivered", "codel_dropped", "unknown_dst", "local_delivered", "blocked")
EOVERFLOW = -75


class SampleRow(C.Structure):
    _fields_ = [("host", C.c_uint32), ("sample", C.c_uint32)] + [(n, C.c_uint64) for n in SAMPLE_FIELDS]


class SampleInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("sample", "rounds", "window_start", "window_end", "first_row", "rows")] + \
               [("total", C.c_uint64 * 7)]


class SampleTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("kernel_ms", C.c_double * 3), ("copy_ms", C.c_double),
                ("hosts", C.c_uint64), ("rows", C.c_uint64)]


SAMPLE_ROW_DTYPE = np.dtype([("host", "<u4"), ("sample", "<u4")] + [(n, "<u8") for n in SAMPLE_FIELDS])
SAMPLE_INFO_DTYPE = np.dtype([(n, "<u8") for n in ("sample", "rounds", "window_start", "window_end", "first_row", "rows")] +
                             [("total", "<u8", (7,))])
assert SAMPLE_ROW_DTYPE.itemsize == C.sizeof(SampleRow) == 64
assert SAMPLE_INFO_DTYPE.itemsize == C.sizeof(SampleInfo) == 104


BACKLOG_ROUTER_HELD, BACKLOG_OUT_HELD = 1, 2
# sgn_backlog_info::total, in order
BACKLOG_TOTALS = ("router_packets", "router_bytes", "router_held", "send_packets", "send_bytes", "out_held",
                  "inflight_packets", "submit_pending")
_BACKLOG_ROW = [("host", "u4"), ("flags", "u4"), ("router_packets", "u4"), ("send_packets", "u4"), ("router_bytes", "u8"),
                ("send_bytes", "u8"), ("router_oldest", "u8"), ("inflight_packets", "u4"), ("submit_pending", "u4"),
                ("inflight_earliest", "u8"), ("inflight_latest", "u8")]
_BACKLOG_INFO = [("rounds", "u8"), ("window_start", "u8"), ("window_end", "u8"), ("hosts", "u8"), ("rows", "u8"),
                 ("total", "u8", 8), ("max_router_packets", "u8"), ("max_router_host", "u4"), ("pad0", "u4"),
                 ("max_sojourn_ns", "u8"), ("max_sojourn_host", "u4"), ("pad1", "u4"), ("inflight_earliest", "u8")]
_CT = {"u4": C.c_uint32, "u8": C.c_uint64}


class BacklogRow(C.Structure):
    _fields_ = [(n, _CT[t]) for n, t in _BACKLOG_ROW]


class BacklogInfo(C.Structure):
    _fields_ = [(f[0], _CT[f[1]] * f[2] if len(f) > 2 else _CT[f[1]]) for f in _BACKLOG_INFO]


class BacklogTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("kernel_ms", C.c_double * 4), ("copy_ms", C.c_double),
                ("hosts", C.c_uint64), ("rows", C.c_uint64), ("calendar_runs", C.c_uint64)]


BACKLOG_ROW_DTYPE = np.dtype([(n, "<" + t) for n, t in _BACKLOG_ROW])
BACKLOG_INFO_DTYPE = np.dtype([(f[0], "<" + f[1], (f[2],)) if len(f) > 2 else (f[0], "<" + f[1]) for f in _BACKLOG_INFO])
assert BACKLOG_ROW_DTYPE.itemsize == C.sizeof(BacklogRow) == 64
assert BACKLOG_INFO_DTYPE.itemsize == C.sizeof(BacklogInfo) == 144


DIGEST_DTYPE = np.dtype([("tx", "<u8"), ("rx", "<u8"), ("app", "<u8"), ("rng", "<u8", (4,)),
                         ("next_event_id", "<u8"), ("n_sent", "<u8"), ("n_popped", "<u8"),
                         ("n_delivered", "<u8"), ("n_codel_dropped", "<u8")])


class PktSoa(C.Structure):
    _fields_ = [("n", C.c_uint64), ("src_host", u32p), ("dst_ip", u32p), ("payload_len", u32p),
                ("wire_len", u32p), ("send_time", u64p), ("handle", u64p)]


class DrainRec(C.Structure):
    _fields_ = [("time", C.c_uint64), ("src_eid", C.c_uint64), ("handle", C.c_uint64),
                ("host", C.c_uint32), ("src_host", C.c_uint32), ("dst_host", C.c_uint32),
                ("status", C.c_uint32), ("payload_len", C.c_uint32), ("tag", C.c_uint32)]


DRAIN_DTYPE = np.dtype([("time", "<u8"), ("src_eid", "<u8"), ("handle", "<u8"), ("host", "<u4"),
                        ("src_host", "<u4"), ("dst_host", "<u4"), ("status", "<u4"),
                        ("payload_len", "<u4"), ("tag", "<u4")])
assert DRAIN_DTYPE.itemsize == C.sizeof(DrainRec)


class DrainTakeTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("kernel_ms", C.c_double * 4), ("copy_ms", C.c_double),
                ("records", C.c_uint64), ("hosts", C.c_uint64), ("largest_span", C.c_uint64),
                ("spans_by_class", C.c_uint64 * 3), ("wave_max", C.c_uint32), ("tile", C.c_uint32)]


DELAY_BINS = 48
# sgn_delay_info::total, in order
DELAY_TOTALS = ("delivered", "dropped", "delay_sum_delivered", "delay_sum_dropped", "standing", "unmatched")
_DELAY_ROW = [("host", "u4"), ("reserved", "u4"), ("standing", "u4"), ("unmatched", "u4"), ("delivered", "u8"), ("dropped", "u8"),
              ("delay_sum_delivered", "u8"), ("delay_sum_dropped", "u8"), ("delay_max", "u8"), ("standing_oldest", "u8")]
_DELAY_INFO = [("rounds", "u8"), ("window_start", "u8"), ("window_end", "u8"), ("folds", "u8"), ("records", "u8"),
               ("hosts", "u8"), ("rows", "u8"), ("total", "u8", 6), ("delay_max", "u8"), ("delay_max_host", "u4"),
               ("pad0", "u4"), ("hist_delivered", "u8", DELAY_BINS), ("hist_dropped", "u8", DELAY_BINS)]


class DelayRow(C.Structure):
    _fields_ = [(n, {"u4": C.c_uint32, "u8": C.c_uint64}[t]) for n, t in _DELAY_ROW]


class DelayInfo(C.Structure):
    _fields_ = [(f[0], {"u4": C.c_uint32, "u8": C.c_uint64}[f[1]] * f[2] if len(f) > 2 else {"u4": C.c_uint32, "u8": C.c_uint64}[f[1]])
                for f in _DELAY_INFO]


class DelayTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("order_ms", C.c_double * 3), ("kernel_ms", C.c_double * 5),
                ("records", C.c_uint64), ("hosts", C.c_uint64), ("largest_span", C.c_uint64), ("carry_entries", C.c_uint64),
                ("spans_by_class", C.c_uint64 * 2), ("wave_max", C.c_uint32), ("tile", C.c_uint32)]


DELAY_ROW_DTYPE = np.dtype([(n, "<" + t) for n, t in _DELAY_ROW])
assert DELAY_ROW_DTYPE.itemsize == C.sizeof(DelayRow) == 64
assert C.sizeof(DelayInfo) == 120 + 16 * DELAY_BINS


def delay_bin_edges():
    """The upper edges of the DELAY_BINS histogram bins, in ns: bin 0 holds delay == 0 (edge 0), bin k
    2^(k-1) <= delay < 2^k (edge 2^k - 1), the last bin everything above (edge: the largest u64)."""
    return [0] + [(1 << k) - 1 for k in range(1, DELAY_BINS - 1)] + [EMUTIME_INVALID]


def pkt_soa(src_host, dst_ip, payload_len, send_time, handle=None, wire_len=None):
    """(PktSoa, keep-alive arrays) for sgn_submit / ora_sim_submit."""
    a = [np.ascontiguousarray(src_host, dtype=np.uint32), np.ascontiguousarray(dst_ip, dtype=np.uint32),
         np.ascontiguousarray(payload_len, dtype=np.uint32), np.ascontiguousarray(send_time, dtype=np.uint64)]
    h = None if handle is None else np.ascontiguousarray(handle, dtype=np.uint64)
    w = None if wire_len is None else np.ascontiguousarray(wire_len, dtype=np.uint32)
    b = PktSoa(len(a[0]), ptr(a[0], C.c_uint32), ptr(a[1], C.c_uint32), ptr(a[2], C.c_uint32),
               ptr(w, C.c_uint32) if w is not None else None, ptr(a[3], C.c_uint64),
               ptr(h, C.c_uint64) if h is not None else None)
    return b, (a, h, w)
assert TRACE_DTYPE.itemsize == C.sizeof(TraceRec)
assert DIGEST_DTYPE.itemsize == C.sizeof(HostDigest)


class CreateOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_rank", C.c_uint32),
                ("shard_count", C.c_uint32), ("flags", C.c_uint32)]


class RoutesTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("latency_ms", C.c_double), ("loss_ms", C.c_double),
                ("loss_iters", C.c_uint32), ("tile", C.c_uint32), ("n_tight_edges", C.c_uint64),
                ("latency_passes", C.c_uint32), ("latency_u64", C.c_uint32),
                ("loss_multi", C.c_uint32), ("latency_bf", C.c_uint32),
                ("shards", C.c_uint32), ("shard_sources", C.c_uint32),
                ("loss_dense", C.c_uint32), ("loss_fused", C.c_uint32)]


class EngineInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "calendar_buckets", "bucket_width_ns", "host_groups", "slab_capacity", "hosts_per_wave",
        "persistent_grid", "persistent_fallbacks", "device_bytes", "exchange_slot_runs",
        "exchange_send_runs", "exchange_hwm_runs", "exchange_spills", "exchange_bytes", "codel_pages",
        "codel_page_allocs", "codel_pages_free", "codel_pages_chained",
        "compute_units", "bucket_min_lds", "lds_per_cu", "codel_pool_grows", "calendar_grows",
        "calendar_spill_runs", "exchange_slot_grows", "rounds_held", "slab_extensions",
        "slab_extension_runs", "big_slab_pieces", "spill_area_runs", "spill_area_grows",
        "exchange_mode", "inbox_slot_runs", "inbox_grows", "inbox_overflow_rounds", "inbox_moved_runs",
        "persistent_x_launches", "persistent_x_grid")]


class SnapshotInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rounds", "window_start", "window_end", "device_bytes", "host_bytes", "calendar_runs",
        "calendar_bytes", "calendar_pool_bytes")] + [("save_ms", C.c_double), ("pack_ms", C.c_double)]


class SnapshotFileInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "format", "abi", "layout_sig", "identity", "rounds", "window_start", "window_end", "file_bytes",
        "n_sections", "calendar_runs", "trace_records")] + [("shard_rank", C.c_uint32), ("shard_count", C.c_uint32)]


class SnapshotFileTiming(C.Structure):
    _fields_ = [("total_ms", C.c_double), ("stream_ms", C.c_double), ("digest_ms", C.c_double),
                ("device_bytes", C.c_uint64), ("file_bytes", C.c_uint64)]


EFILE = -74
WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)  # sgn_write_fn
READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)   # sgn_read_fn


class KernelTimes(C.Structure):
    _fields_ = [("launches", C.c_uint64 * 16), ("ms", C.c_double * 16),
                ("name", C.c_char_p * 16), ("n_kernels", C.c_uint32),
                ("launches_total", C.c_uint64 * 16)]


_lib = None


def build_id() -> str:
    """A fingerprint of the libsgn sources the shipped libsgn.so is built from (csrc/ and the
    public headers): measurements filed under profiles/ carry it, and bench.py quotes a
    measurement only for the build it was taken on."""
    import hashlib
    here = pathlib.Path(__file__).resolve().parent
    files = sorted(list((here / "csrc").glob("*.hip")) + list((here / "csrc").glob("*.cpp")) +
                   list((here / "csrc").glob("*.h")) + [here / "csrc" / "Makefile"] +
                   list((here.parent / "include").glob("*.h")))
    h = hashlib.sha256()
    for f in files:
        h.update(f.name.encode() + b"\0" + f.read_bytes() + b"\0")
    return h.hexdigest()[:16]


def load(path: str | os.PathLike | None = None) -> C.CDLL:
    """Load libsgn.so (raises if it was not built: the product has no fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = pathlib.Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(f"libsgn not built: {p} missing (run __graft_entry__.build())")
    L = C.CDLL(str(p))
    vp = C.c_void_p
    sig = {
        "sgn_create": (C.c_int, [C.POINTER(vp), C.POINTER(CreateOpts)]),
        "sgn_destroy": (None, [vp]),
        "sgn_last_error": (C.c_char_p, [vp]),
        "sgn_abi_version": (C.c_int, []),
        "sgn_routes_build": (C.c_int, [vp, C.POINTER(Graph), u32p, C.c_uint32, C.c_int32]),
        "sgn_route_get": (C.c_int, [vp, C.c_uint32, C.c_uint32, u64p, f32p]),
        "sgn_routes_copy": (C.c_int, [vp, u64p, f32p]),
        "sgn_min_latency": (C.c_int, [vp, u64p]),
        "sgn_routes_timing_get": (C.c_int, [vp, C.POINTER(RoutesTiming)]),
        "sgn_hosts_set": (C.c_int, [vp, C.POINTER(Hosts)]),
        "sgn_derive_host_seeds": (C.c_int, [C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, u64p]),
        "sgn_sim_init": (C.c_int, [vp, C.POINTER(SimConfig), C.POINTER(Traffic)]),
        "sgn_window": (C.c_int, [vp, u64p, u64p, C.POINTER(C.c_int32)]),
        "sgn_round": (C.c_int, [vp, u64p]),
        "sgn_run": (C.c_int, [vp, C.c_uint64, u64p]),
        "sgn_stats_get": (C.c_int, [vp, C.POINTER(Stats)]),
        "sgn_host_digests": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(HostDigest)]),
        "sgn_host_next_event_time": (C.c_int, [vp, C.c_uint32, u64p]),
        "sgn_trace_enable": (C.c_int, [vp, C.c_uint64]),
        "sgn_trace_read": (C.c_int, [vp, C.POINTER(TraceRec), C.c_uint64, u64p]),
        "sgn_kernel_times_get": (C.c_int, [vp, C.POINTER(KernelTimes)]),
        "sgn_engine_info_get": (C.c_int, [vp, C.POINTER(EngineInfo)]),
        "sgn_comm_get_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
        "sgn_comm_init": (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_uint64]),
        "sgn_shard_range": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]),
        "sgn_comm_init_local": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64]),
        "sgn_run_local_group": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64, u64p]),
        "sgn_worker_get_latency": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
        "sgn_worker_is_routable": (C.c_int32, [vp, C.c_uint32, C.c_uint32]),
        "sgn_worker_get_bandwidth_up_bytes": (C.c_uint64, [vp, C.c_uint32]),
        "sgn_worker_get_bandwidth_down_bytes": (C.c_uint64, [vp, C.c_uint32]),
        "sgn_addr_to_host_id": (C.c_int, [vp, C.c_uint32, u32p]),
        "sgn_gml_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(vp), C.c_char_p, C.c_size_t]),
        "sgn_gml_free": (None, [vp]),
        "sgn_gml_graph": (C.c_int, [vp, C.POINTER(Graph)]),
        "sgn_gml_node_bandwidth": (C.c_int, [vp, C.c_uint32, u64p, C.POINTER(C.c_int32), u64p,
                                             C.POINTER(C.c_int32)]),
        "sgn_units_parse": (C.c_int, [C.c_int32, C.c_char_p, u64p]),
        "sgn_assign_ips": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint8), u32p, u32p]),
        "sgn_pcap_open": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(vp)]),
        "sgn_pcap_write_packet": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32]),
        "sgn_pcap_close": (C.c_int, [vp]),
        "sgn_packet_bytes": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_uint8), C.c_uint32]),
        "sgn_trace_pcap": (C.c_int64, [C.POINTER(TraceRec), C.c_uint64, C.c_uint32, u32p, C.c_uint32,
                                       C.c_char_p, C.c_uint32]),
        "sgn_selftest_codel_law": (C.c_int, [vp, C.c_uint64, u64p]),
        "sgn_selftest_report_scan": (C.c_int, [vp, u32p, C.c_uint32, u32p, u64p]),
        "sgn_debug_stamps": (C.c_int, [vp, u64p, C.c_uint64, u64p]),
        "sgn_debug_rounds": (C.c_int, [vp, u64p]),
        "sgn_debug_rounds_x": (C.c_int, [vp, u64p]),
        "sgn_debug_rounds_xw": (C.c_int, [vp, u64p]),
        "sgn_submit": (C.c_int, [vp, C.POINTER(PktSoa)]),
        "sgn_drain_enable": (C.c_int, [vp, C.c_uint64]),
        "sgn_drain": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.POINTER(DrainRec), C.c_uint64, u64p]),
        "sgn_drain_pending": (C.c_int, [vp, u64p]),
        "sgn_drain_take": (C.c_int, [vp, C.POINTER(DrainRec), C.c_uint64, u64p, C.POINTER(TraceSpan), C.c_uint64, u64p]),
        "sgn_drain_take_timing_get": (C.c_int, [vp, C.POINTER(DrainTakeTiming)]),
        "sgn_selftest_drain_order": (C.c_int, [vp, C.POINTER(DrainRec), C.c_uint64, C.c_uint32, C.c_uint32,
                                               C.POINTER(DrainRec), C.POINTER(TraceSpan), C.c_uint64, u64p]),
        "sgn_set_window": (C.c_int, [vp, C.c_uint64, C.c_uint64]),
        "sgn_rng_next_u64": (C.c_int, [vp, C.c_uint32, u64p]),
        "sgn_rng_double": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_double)]),
        "sgn_rng_fill_bytes": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t]),
        "sgn_rng_next_u64_batch": (C.c_int, [vp, u32p, u32p, C.c_uint32, u64p]),
        "sgn_hosts_next_event_time": (C.c_int, [vp, C.c_uint32, C.c_uint32, u64p]),
        "sgn_stage_create": (C.c_int, [vp, C.POINTER(vp)]),
        "sgn_stage_destroy": (None, [vp]),
        "sgn_stage_push": (C.c_int, [vp, C.POINTER(PktSoa)]),
        "sgn_stage_pending": (C.c_uint64, [vp]),
        "sgn_stage_flush": (C.c_int, [vp]),
        "sgn_run_until": (C.c_int, [vp, C.c_uint64, u64p]),
        "sgn_snapshot_save": (C.c_int, [vp, C.POINTER(vp)]),
        "sgn_snapshot_restore": (C.c_int, [vp, vp]),
        "sgn_snapshot_free": (None, [vp, vp]),
        "sgn_snapshot_info_get": (C.c_int, [vp, C.POINTER(SnapshotInfo)]),
        "sgn_shards_run_until": (C.c_int, [C.POINTER(vp), C.c_uint32, C.c_uint64, u64p]),
        "sgn_shards_snapshot_save": (C.c_int, [C.POINTER(vp), C.c_uint32, C.POINTER(vp)]),
        "sgn_shards_snapshot_restore": (C.c_int, [C.POINTER(vp), C.c_uint32, C.POINTER(vp)]),
        "sgn_snapshot_export": (C.c_int, [vp, vp, WRITE_FN, vp, u64p]),
        "sgn_snapshot_import": (C.c_int, [vp, READ_FN, vp, C.POINTER(vp)]),
        "sgn_snapshot_export_file": (C.c_int, [vp, vp, C.c_char_p, u64p]),
        "sgn_snapshot_import_file": (C.c_int, [vp, C.c_char_p, C.POINTER(vp)]),
        "sgn_snapshot_file_info_get": (C.c_int, [C.c_char_p, C.POINTER(SnapshotFileInfo)]),
        "sgn_snapshot_file_timing_get": (C.c_int, [vp, C.POINTER(SnapshotFileTiming)]),
        "sgn_digest_bytes": (C.c_uint64, [vp, C.c_size_t]),
        "sgn_selftest_digest": (C.c_int, [vp, vp, C.c_size_t, u64p]),
        "sgn_trace_hosts": (C.c_int, [vp, u32p, C.c_uint32]),
        "sgn_trace_pending": (C.c_int, [vp, u64p]),
        "sgn_trace_take": (C.c_int, [vp, C.POINTER(TraceRec), C.c_uint64, u64p, C.POINTER(TraceSpan), C.c_uint64, u64p]),
        "sgn_trace_take_timing_get": (C.c_int, [vp, C.POINTER(TraceTakeTiming)]),
        "sgn_pcap_write_trace": (C.c_int64, [vp, C.POINTER(TraceRec), C.c_uint64, C.c_uint32, u32p, C.c_uint32]),
        "sgn_sample_enable": (C.c_int, [vp, C.c_uint64]),
        "sgn_sample": (C.c_int, [vp, C.POINTER(SampleInfo)]),
        "sgn_sample_rebase": (C.c_int, [vp]),
        "sgn_sample_pending": (C.c_int, [vp, u64p, u64p]),
        "sgn_sample_take": (C.c_int, [vp, C.POINTER(SampleRow), C.c_uint64, u64p, C.POINTER(SampleInfo), C.c_uint64, u64p]),
        "sgn_sample_timing_get": (C.c_int, [vp, C.POINTER(SampleTiming)]),
        "sgn_backlog": (C.c_int, [vp, C.POINTER(BacklogRow), C.c_uint64, u64p, C.POINTER(BacklogInfo)]),
        "sgn_backlog_timing_get": (C.c_int, [vp, C.POINTER(BacklogTiming)]),
        "sgn_delay_enable": (C.c_int, [vp]),
        "sgn_delay_fold": (C.c_int, [vp, C.POINTER(DelayInfo)]),
        "sgn_delay_get": (C.c_int, [vp, C.POINTER(DelayRow), C.c_uint64, u64p, C.POINTER(DelayInfo)]),
        "sgn_delay_clear": (C.c_int, [vp]),
        "sgn_delay_timing_get": (C.c_int, [vp, C.POINTER(DelayTiming)]),
        "sgn_selftest_delay_fold": (C.c_int, [vp, C.POINTER(TraceRec), u64p, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                              C.POINTER(DelayRow), C.c_uint64, u64p, C.POINTER(DelayInfo)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if path is None:
        _lib = L
    return L


def ptr(a: np.ndarray, ct):
    return a.ctypes.data_as(C.POINTER(ct))


class SgnError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__(f"libsgn error {rc}: {msg}")
        self.rc = rc


class GraphArrays:
    """Keeps numpy arrays alive behind an sgn_graph struct."""

    def __init__(self, node_id, src, dst, lat, loss, directed):
        self.node_id = np.ascontiguousarray(node_id, dtype=np.uint32)
        self.src = np.ascontiguousarray(src, dtype=np.uint32)
        self.dst = np.ascontiguousarray(dst, dtype=np.uint32)
        self.lat = np.ascontiguousarray(lat, dtype=np.uint64)
        self.loss = np.ascontiguousarray(loss, dtype=np.float32)
        self.directed = int(directed)

    def struct(self) -> Graph:
        return Graph(len(self.node_id), ptr(self.node_id, C.c_uint32), len(self.src),
                     ptr(self.src, C.c_uint32), ptr(self.dst, C.c_uint32),
                     ptr(self.lat, C.c_uint64), ptr(self.loss, C.c_float), self.directed)


class HostArrays:
    def __init__(self, ip, node_id, bw_up, bw_down, seed):
        self.ip = np.ascontiguousarray(ip, dtype=np.uint32)
        self.node_id = np.ascontiguousarray(node_id, dtype=np.uint32)
        self.bw_up = np.ascontiguousarray(bw_up, dtype=np.uint64)
        self.bw_down = np.ascontiguousarray(bw_down, dtype=np.uint64)
        self.seed = np.ascontiguousarray(seed, dtype=np.uint64)

    @property
    def n(self):
        return len(self.ip)

    def struct(self) -> Hosts:
        return Hosts(len(self.ip), ptr(self.ip, C.c_uint32), ptr(self.node_id, C.c_uint32),
                     ptr(self.bw_up, C.c_uint64), ptr(self.bw_down, C.c_uint64),
                     ptr(self.seed, C.c_uint64))


def make_traffic(kind=TRAFFIC_PERIODIC, *, flow_seed=7, start_ns=0, start_jitter_ns=0,
                 period_ns=10_000_000, period_jitter_ns=0, payload_len=1024,
                 unknown_dst_permille=0, req_payload=64, servers=None,
                 file_bytes=(50 * 1024, 1024 * 1024, 5 * 1024 * 1024)):
    t = Traffic()
    t.kind = kind
    t.payload_len = payload_len
    t.flow_seed = flow_seed
    t.start_ns = start_ns
    t.start_jitter_ns = start_jitter_ns
    t.period_ns = period_ns
    t.period_jitter_ns = period_jitter_ns
    t.unknown_dst_permille = unknown_dst_permille
    t.req_payload = req_payload
    keep = None
    if servers is not None:
        keep = np.ascontiguousarray(servers, dtype=np.uint32)
        t.n_servers = len(keep)
        t.server_hosts = ptr(keep, C.c_uint32)
    for i in range(3):
        t.file_bytes[i] = int(file_bytes[i])
    t._keep = keep  # noqa: SLF001 keep the server array alive with the struct
    return t


def make_config(stop_time_ns, *, bootstrap_end_ns=0, runahead_ns=1_000_000, dynamic=False,
                out_fifo_cap=64, codel_cap=1024, event_capacity=0, qdisc=0):
    c = SimConfig()
    c.stop_time_ns = stop_time_ns
    c.bootstrap_end_ns = bootstrap_end_ns
    c.runahead_ns = runahead_ns
    c.use_dynamic_runahead = 1 if dynamic else 0
    c.out_fifo_cap = out_fifo_cap
    c.codel_cap = codel_cap
    c.event_capacity = event_capacity
    c.interface_qdisc = qdisc
    return c


class Context:
    """One libsgn context (one GPU / shard)."""

    def __init__(self, device=0, shard_rank=0, shard_count=1, flags=0, lib=None):
        self.L = lib or load()
        self.h = C.c_void_p()
        opts = CreateOpts(device, shard_rank, shard_count, flags)
        rc = self.L.sgn_create(C.byref(self.h), C.byref(opts))
        if rc != 0:
            raise SgnError(rc, self.L.sgn_last_error(None).decode())
        self._keep = []

    def check(self, rc):
        if rc != 0:
            raise SgnError(rc, self.L.sgn_last_error(self.h).decode())
        return rc

    def close(self):
        if self.h:
            self.L.sgn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- routing ----
    def routes_build(self, g: GraphArrays, used_node_ids, shortest=True):
        used = np.ascontiguousarray(used_node_ids, dtype=np.uint32)
        gs = g.struct()
        self.check(self.L.sgn_routes_build(self.h, C.byref(gs), ptr(used, C.c_uint32),
                                           len(used), 1 if shortest else 0))
        self.U = len(used)

    def routes_copy(self):
        lat = np.zeros(self.U * self.U, dtype=np.uint64)
        loss = np.zeros(self.U * self.U, dtype=np.float32)
        self.check(self.L.sgn_routes_copy(self.h, ptr(lat, C.c_uint64), ptr(loss, C.c_float)))
        return lat.reshape(self.U, self.U), loss.reshape(self.U, self.U)

    def routes_timing(self):
        t = RoutesTiming()
        self.check(self.L.sgn_routes_timing_get(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    # ---- hosts / sim ----
    def hosts_set(self, hosts: HostArrays):
        self._hosts = hosts
        hs = hosts.struct()
        self.check(self.L.sgn_hosts_set(self.h, C.byref(hs)))

    def trace_enable(self, cap):
        self.check(self.L.sgn_trace_enable(self.h, cap))

    def sim_init(self, cfg: SimConfig, traffic: Traffic):
        self._traffic = traffic
        self.check(self.L.sgn_sim_init(self.h, C.byref(cfg), C.byref(traffic)))

    def window(self):
        s, e, a = C.c_uint64(), C.c_uint64(), C.c_int32()
        self.check(self.L.sgn_window(self.h, C.byref(s), C.byref(e), C.byref(a)))
        return s.value, e.value, bool(a.value)

    def round(self):
        m = C.c_uint64()
        self.check(self.L.sgn_round(self.h, C.byref(m)))
        return m.value

    def run(self, max_rounds=1 << 62):
        d = C.c_uint64()
        self.check(self.L.sgn_run(self.h, max_rounds, C.byref(d)))
        return d.value

    # ---- run-control: run to a simulated time, snapshot, rewind (single shard) ----
    def run_until(self, t_emulated):
        """Whole windows until the next one would start at or after t_emulated (EmulatedTime);
        returns the rounds run."""
        d = C.c_uint64()
        self.check(self.L.sgn_run_until(self.h, t_emulated, C.byref(d)))
        return d.value

    def snapshot_save(self):
        """A handle to a snapshot of the simulation as it is now (owned by this context)."""
        s = C.c_void_p()
        self.check(self.L.sgn_snapshot_save(self.h, C.byref(s)))
        return s

    def snapshot_restore(self, snap):
        self.check(self.L.sgn_snapshot_restore(self.h, snap))

    def snapshot_free(self, snap):
        self.L.sgn_snapshot_free(self.h, snap)

    def snapshot_info(self, snap):
        i = SnapshotInfo()
        rc = self.L.sgn_snapshot_info_get(snap, C.byref(i))
        if rc != 0:
            raise SgnError(rc, "sgn_snapshot_info_get: null argument")
        return {n: getattr(i, n) for n, _ in i._fields_}

    # ---- snapshot files: a snapshot out of this context and process, and into a fresh one ----
    def snapshot_export(self, snap, path):
        """Writes snap to path (through path.tmp and a rename); returns the file's length."""
        n = C.c_uint64()
        self.check(self.L.sgn_snapshot_export_file(self.h, snap, os.fsencode(path), C.byref(n)))
        return n.value

    def snapshot_import(self, path):
        """A new snapshot of this context from a file written by a simulation made by the same
        calls; nothing else changes until snapshot_restore (or shards_snapshot_restore)."""
        s = C.c_void_p()
        self.check(self.L.sgn_snapshot_import_file(self.h, os.fsencode(path), C.byref(s)))
        return s

    def snapshot_export_stream(self, snap, write):
        """The stream form: write(bytes) is called in file order; a false return or an exception
        ends the export with EFILE. Returns the stream's length."""
        def cb(_user, data, n):
            try:
                return 0 if write(C.string_at(data, n)) is not False else 1
            except Exception:  # noqa: BLE001 (nothing may unwind across the C ABI)
                return 1
        n = C.c_uint64()
        self.check(self.L.sgn_snapshot_export(self.h, snap, WRITE_FN(cb), None, C.byref(n)))
        return n.value

    def snapshot_import_stream(self, read):
        """The stream form: read(n) returns exactly n bytes (fewer: EFILE)."""
        def cb(_user, data, n):
            try:
                b = read(n)
            except Exception:  # noqa: BLE001
                return 1
            if b is None or len(b) != n:
                return 1
            C.memmove(data, b, n)
            return 0
        s = C.c_void_p()
        self.check(self.L.sgn_snapshot_import(self.h, READ_FN(cb), None, C.byref(s)))
        return s

    def snapshot_file_timing(self):
        t = SnapshotFileTiming()
        self.check(self.L.sgn_snapshot_file_timing_get(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in t._fields_}

    def selftest_digest(self, buf):
        """The section digest of buf (bytes-like, a multiple of 4 bytes) by the device kernel."""
        a = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        out = C.c_uint64()
        self.check(self.L.sgn_selftest_digest(self.h, a.ctypes.data if a.size else None, a.size, C.byref(out)))
        return out.value

    def stats(self):
        s = Stats()
        self.check(self.L.sgn_stats_get(self.h, C.byref(s)))
        return s.as_dict()

    def digests(self, lo, hi):
        out = np.zeros(hi - lo, dtype=DIGEST_DTYPE)
        self.check(self.L.sgn_host_digests(self.h, lo, hi, out.ctypes.data_as(C.POINTER(HostDigest))))
        return out

    def trace(self):
        """The records in the trace buffer, unordered: all of them, or after trace_take() those
        produced since the last take."""
        n = C.c_uint64()
        self.check(self.L.sgn_trace_pending(self.h, C.byref(n)))
        out = np.zeros(n.value, dtype=TRACE_DTYPE)
        self.check(self.L.sgn_trace_read(self.h, out.ctypes.data_as(C.POINTER(TraceRec)), n.value, C.byref(n)))
        return out

    # ---- a trace of chosen hosts, taken out in ordered pieces (sgn_trace_hosts / _take) ----
    def trace_hosts(self, hosts):
        """After trace_enable and before sim_init: only these HostIds are traced ([] : all)."""
        h = np.ascontiguousarray(hosts, dtype=np.uint32)
        self.check(self.L.sgn_trace_hosts(self.h, ptr(h, C.c_uint32) if len(h) else None, len(h)))

    def trace_pending(self):
        n = C.c_uint64()
        self.check(self.L.sgn_trace_pending(self.h, C.byref(n)))
        return n.value

    def trace_take(self, cap=None, span_cap=None):
        """(records, spans): every record produced and not yet taken, sorted by (host, seq) on the
        device, and one span {host, first, count} per host with records (ascending host); the
        trace buffer is empty afterwards. cap / span_cap: the arrays' sizes (default: what is
        pending); too small raises SgnError with rc ERANGE, .needed = (records, spans), and takes
        nothing."""
        if cap is None:
            cap = self.trace_pending()
        if span_cap is None:
            span_cap = min(cap, self._hosts.n)
        recs = np.zeros(cap, dtype=TRACE_DTYPE)
        spans = np.zeros(span_cap, dtype=SPAN_DTYPE)
        n, ns = C.c_uint64(), C.c_uint64()
        rc = self.L.sgn_trace_take(self.h, recs.ctypes.data_as(C.POINTER(TraceRec)) if cap else None, cap, C.byref(n),
                                   spans.ctypes.data_as(C.POINTER(TraceSpan)) if span_cap else None, span_cap, C.byref(ns))
        if rc != 0:
            e = SgnError(rc, self.L.sgn_last_error(self.h).decode())
            e.needed = (n.value, ns.value)
            raise e
        return recs[: n.value], spans[: ns.value]

    def trace_take_timing(self):
        t = TraceTakeTiming()
        self.check(self.L.sgn_trace_take_timing_get(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "kernel_ms": list(t.kernel_ms), "copy_ms": t.copy_ms,
                "records": t.records, "hosts": t.hosts}

    # ---- interval statistics: per-host counter deltas sampled on the device (sgn_sample_*) ----
    def sample_enable(self, row_capacity):
        """After sim_init: a device buffer of row_capacity rows and a baseline of the per-host
        counters as they are now; the sample index starts at 0."""
        self.check(self.L.sgn_sample_enable(self.h, row_capacity))
        self.sample_capacity = int(row_capacity)

    def sample(self):
        """One sample at the round edge the context is at: a row (counters - baseline) for every
        owned host that changed, ascending by host, appended on the device. Returns the sample's
        info as a dict (total: the seven sums in SAMPLE_FIELDS order). SgnError with rc EOVERFLOW
        when the row buffer has too few free rows (nothing changed: sample_take(), then again)."""
        i = SampleInfo()
        self.check(self.L.sgn_sample(self.h, C.byref(i)))
        d = {n: int(getattr(i, n)) for n, _ in i._fields_ if n != "total"}
        d["total"] = [int(v) for v in i.total]
        return d

    def sample_rebase(self):
        """The baseline := the counters as they are now (after a rewind behind it); emits nothing."""
        self.check(self.L.sgn_sample_rebase(self.h))

    def sample_pending(self):
        """(rows, samples) appended and not yet taken."""
        r, s = C.c_uint64(), C.c_uint64()
        self.check(self.L.sgn_sample_pending(self.h, C.byref(r), C.byref(s)))
        return r.value, s.value

    def sample_take(self, cap=None, info_cap=None):
        """(rows, infos) as arrays of SAMPLE_ROW_DTYPE / SAMPLE_INFO_DTYPE: every pending row,
        ordered by sample, then host, and the pending samples' infos (infos[k]'s rows are
        rows[first_row : first_row + rows]); the row buffer is empty afterwards. cap / info_cap: the
        arrays' sizes (default: what is pending); too small raises SgnError with rc ERANGE,
        .needed = (rows, samples), and takes nothing."""
        pr, ps = self.sample_pending()
        cap = pr if cap is None else cap
        info_cap = ps if info_cap is None else info_cap
        rows = np.zeros(cap, dtype=SAMPLE_ROW_DTYPE)
        infos = np.zeros(info_cap, dtype=SAMPLE_INFO_DTYPE)
        n, ni = C.c_uint64(), C.c_uint64()
        rc = self.L.sgn_sample_take(self.h, rows.ctypes.data_as(C.POINTER(SampleRow)) if cap else None, cap, C.byref(n),
                                    infos.ctypes.data_as(C.POINTER(SampleInfo)) if info_cap else None, info_cap, C.byref(ni))
        if rc != 0:
            e = SgnError(rc, self.L.sgn_last_error(self.h).decode())
            e.needed = (n.value, ni.value)
            raise e
        return rows[: n.value], infos[: ni.value]

    def sample_timing(self):
        t = SampleTiming()
        self.check(self.L.sgn_sample_timing_get(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "kernel_ms": list(t.kernel_ms), "copy_ms": t.copy_ms,
                "hosts": t.hosts, "rows": t.rows}

    # ---- the backlog report: standing queues and in-flight packets per owned host (sgn_backlog) ----
    def backlog(self, rows=True, cap=None):
        """What stands in the network at the round edge the context is at, as a Backlog: .info (the
        totals and maxima, folded on the device) and .rows (BACKLOG_ROW_DTYPE, one per owned host
        with anything standing, ascending by host). rows=False asks for the totals only (no row is
        copied; info["rows"] still counts them). cap: the row array's size (default: the row
        count, asked for first); too small raises SgnError with rc ERANGE, .needed = the row
        count and .info = the info, which is filled all the same."""
        info = BacklogInfo()
        n = C.c_uint64()
        if cap is None:
            self.check(self.L.sgn_backlog(self.h, None, 0, C.byref(n), C.byref(info)))
            if not rows or n.value == 0:
                return Backlog(info, None)
            cap = n.value
        out = np.zeros(cap, dtype=BACKLOG_ROW_DTYPE)
        rc = self.L.sgn_backlog(self.h, out.ctypes.data_as(C.POINTER(BacklogRow)) if cap else None, cap, C.byref(n),
                                C.byref(info))
        if rc != 0:
            e = SgnError(rc, self.L.sgn_last_error(self.h).decode())
            e.needed = n.value
            e.info = Backlog(info, None).info
            e.out = out
            raise e
        return Backlog(info, out[: n.value] if rows else None)

    def backlog_timing(self):
        t = BacklogTiming()
        self.check(self.L.sgn_backlog_timing_get(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "kernel_ms": list(t.kernel_ms), "copy_ms": t.copy_ms,
                "hosts": t.hosts, "rows": t.rows, "calendar_runs": t.calendar_runs}

    # ---- the router delay report: queueing delay per packet, folded on the device (sgn_delay_*) ----
    def delay_enable(self):
        """After sim_init on a traced context with no trace record pending: starts the report from
        the state as it is now (what stands at a router becomes unknown carry entries)."""
        self.check(self.L.sgn_delay_enable(self.h))

    def delay_fold(self):
        """A take whose records stay on the device: every pending trace record is ordered, folded
        into the report and dropped. Returns the info as a dict (Delay.info)."""
        info = DelayInfo()
        self.check(self.L.sgn_delay_fold(self.h, C.byref(info)))
        return Delay(info).info

    def delay(self, rows=True, cap=None):
        """The report since the last enable or clear, as a Delay. rows=False: the totals only. cap:
        the row array's size (default: the row count, asked for first); too small raises SgnError
        with rc ERANGE, .needed = the row count, .info = the info and .out = the untouched array."""
        info = DelayInfo()
        n = C.c_uint64()
        if cap is None:
            self.check(self.L.sgn_delay_get(self.h, None, 0, C.byref(n), C.byref(info)))
            if not rows or n.value == 0:
                return Delay(info, None)
            cap = n.value
        out = np.zeros(cap, dtype=DELAY_ROW_DTYPE)
        rc = self.L.sgn_delay_get(self.h, out.ctypes.data_as(C.POINTER(DelayRow)) if cap else None, cap, C.byref(n), C.byref(info))
        if rc != 0:
            e = SgnError(rc, self.L.sgn_last_error(self.h).decode())
            e.needed = n.value
            e.info = Delay(info).info
            e.out = out
            raise e
        return Delay(info, out[: n.value] if rows else None)

    def delay_clear(self):
        """Zeroes the accumulators and histograms; the carry stays (intervals: delay() + delay_clear())."""
        self.check(self.L.sgn_delay_clear(self.h))

    def delay_timing(self):
        t = DelayTiming()
        self.check(self.L.sgn_delay_timing_get(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "order_ms": list(t.order_ms), "kernel_ms": list(t.kernel_ms), "records": t.records,
                "hosts": t.hosts, "largest_span": t.largest_span, "carry_entries": t.carry_entries,
                "spans_by_class": list(t.spans_by_class), "wave_max": t.wave_max, "tile": t.tile}

    # ---- CPU-resident applications (TRAFFIC_EXTERNAL) and the host RNG ----
    def drain_enable(self, cap):
        self.check(self.L.sgn_drain_enable(self.h, cap))

    def submit(self, src_host, dst_ip, payload_len, send_time, handle=None, wire_len=None):
        b, keep = pkt_soa(src_host, dst_ip, payload_len, send_time, handle, wire_len)
        self.check(self.L.sgn_submit(self.h, C.byref(b)))

    def drain(self, lo=0, hi=0xFFFFFFFF, cap=1 << 22):
        out = np.zeros(cap, dtype=DRAIN_DTYPE)
        n = C.c_uint64()
        self.check(self.L.sgn_drain(self.h, lo, hi, out.ctypes.data_as(C.POINTER(DrainRec)), cap, C.byref(n)))
        return out[: n.value]

    def drain_pending(self):
        """Drain records produced and not yet returned (on the device, or held by an earlier drain)."""
        n = C.c_uint64()
        self.check(self.L.sgn_drain_pending(self.h, C.byref(n)))
        return n.value

    def drain_take(self, cap=None, span_cap=None):
        """(records, spans): EVERY pending drain record, ordered on the device by drain()'s key, and
        one span {host, first, count} per host with records (ascending host). Nothing is pending
        afterwards. By default the arrays are sized from drain_pending() and the call is repeated
        once with the counts an ERANGE carries; with cap / span_cap given, too small raises
        SgnError with rc ERANGE, .needed = (records, spans), and takes nothing."""
        sized = cap is None and span_cap is None
        if cap is None:
            cap = self.drain_pending()
        if span_cap is None:
            span_cap = min(cap, self._hosts.n)
        for attempt in (0, 1):
            recs = np.zeros(cap, dtype=DRAIN_DTYPE)
            spans = np.zeros(span_cap, dtype=SPAN_DTYPE)
            n, ns = C.c_uint64(), C.c_uint64()
            rc = self.L.sgn_drain_take(self.h, recs.ctypes.data_as(C.POINTER(DrainRec)) if cap else None, cap, C.byref(n),
                                       spans.ctypes.data_as(C.POINTER(TraceSpan)) if span_cap else None, span_cap, C.byref(ns))
            if rc == ERANGE and sized and attempt == 0:
                cap, span_cap = n.value, ns.value
                continue
            if rc != 0:
                e = SgnError(rc, self.L.sgn_last_error(self.h).decode())
                e.needed = (n.value, ns.value)
                raise e
            return recs[: n.value], spans[: ns.value]

    def drain_take_timing(self):
        t = DrainTakeTiming()
        self.check(self.L.sgn_drain_take_timing_get(self.h, C.byref(t)))
        return {"total_ms": t.total_ms, "kernel_ms": list(t.kernel_ms), "copy_ms": t.copy_ms, "records": t.records,
                "hosts": t.hosts, "largest_span": t.largest_span, "spans_by_class": list(t.spans_by_class),
                "wave_max": t.wave_max, "tile": t.tile}

    def set_window(self, start, end):
        self.check(self.L.sgn_set_window(self.h, start, end))

    def rng_next_u64(self, host):
        v = C.c_uint64()
        self.check(self.L.sgn_rng_next_u64(self.h, host, C.byref(v)))
        return v.value

    def rng_double(self, host):
        v = C.c_double()
        self.check(self.L.sgn_rng_double(self.h, host, C.byref(v)))
        return v.value

    def rng_fill_bytes(self, host, n):
        buf = (C.c_uint8 * max(1, n))()
        self.check(self.L.sgn_rng_fill_bytes(self.h, host, buf, n))
        return bytes(buf[:n])

    def engine_info(self):
        e = EngineInfo()
        self.check(self.L.sgn_engine_info_get(self.h, C.byref(e)))
        return {n: int(getattr(e, n)) for n, _ in e._fields_}

    def rng_next_u64_batch(self, hosts, counts):
        h = np.ascontiguousarray(hosts, dtype=np.uint32)
        k = np.ascontiguousarray(counts, dtype=np.uint32)
        out = np.zeros(max(1, int(k.sum())), dtype=np.uint64)
        self.check(self.L.sgn_rng_next_u64_batch(self.h, ptr(h, C.c_uint32), ptr(k, C.c_uint32), len(h),
                                                 ptr(out, C.c_uint64)))
        return out[: int(k.sum())]

    def next_event_time(self, host):
        t = C.c_uint64()
        self.check(self.L.sgn_host_next_event_time(self.h, host, C.byref(t)))
        return t.value

    def next_event_times(self, lo, hi):
        out = np.zeros(max(1, hi - lo), dtype=np.uint64)
        self.check(self.L.sgn_hosts_next_event_time(self.h, lo, hi, ptr(out, C.c_uint64)))
        return out[: hi - lo]

    # ---- per-thread staging (sgn_stage_*) ----
    def stage_create(self):
        st = C.c_void_p()
        self.check(self.L.sgn_stage_create(self.h, C.byref(st)))
        return st

    def stage_push(self, st, src_host, dst_ip, payload_len, send_time, handle=None, wire_len=None):
        b, keep = pkt_soa(src_host, dst_ip, payload_len, send_time, handle, wire_len)
        rc = self.L.sgn_stage_push(st, C.byref(b))
        if rc != 0:
            raise SgnError(rc, "sgn_stage_push: invalid batch")

    def stage_flush(self):
        self.check(self.L.sgn_stage_flush(self.h))

    def kernel_times(self):
        k = KernelTimes()
        self.check(self.L.sgn_kernel_times_get(self.h, C.byref(k)))
        return {k.name[i].decode(): (int(k.launches[i]), float(k.ms[i])) for i in range(k.n_kernels)}

    def kernel_launches_total(self):
        """Every launch of each engine kernel since sim_init (kernel_times() covers a sample)."""
        k = KernelTimes()
        self.check(self.L.sgn_kernel_times_get(self.h, C.byref(k)))
        return {k.name[i].decode(): int(k.launches_total[i]) for i in range(k.n_kernels)}


# ------------------------------------------------------------------------------------
# Run-control for sharded simulations. shards: this process's shards, as sgn_shards_* take them —
# every Context of a local group in rank order, or [the one Context of a rank with a communicator]
# (then a collective: every rank makes the same call).
# ------------------------------------------------------------------------------------

def _shard_array(shards):
    return (C.c_void_p * len(shards))(*[c.h.value for c in shards])


def _shards_call(shards, name, *args):
    """fn(ctxs, n, *args); the library reports an error on the context it refused: the one whose
    last error changed speaks."""
    errs = lambda: [c.L.sgn_last_error(c.h).decode() for c in shards]  # noqa: E731
    before = errs()
    rc = getattr(shards[0].L, name)(_shard_array(shards), len(shards), *args)
    if rc != 0:
        after = errs()
        new = [a for a, b in zip(after, before) if a != b] or [a for a in after if a]
        raise SgnError(rc, new[0] if new else name + ": invalid argument")


def selftest_drain_order(ctx, recs, host_lo, n_hosts, span_cap=None):
    """drain_take's kernels on the caller's records (DRAIN_DTYPE) of hosts [host_lo, host_lo +
    n_hosts): (ordered records, spans). Needs no simulation; handle is copied through. An error
    (SgnError) carries the output array as .out and the span count as .needed."""
    recs = np.ascontiguousarray(recs, dtype=DRAIN_DTYPE)
    n = len(recs)
    span_cap = min(n, n_hosts) if span_cap is None else span_cap
    out = np.zeros(n, dtype=DRAIN_DTYPE)
    spans = np.zeros(span_cap, dtype=SPAN_DTYPE)
    ns = C.c_uint64()
    rc = ctx.L.sgn_selftest_drain_order(ctx.h, recs.ctypes.data_as(C.POINTER(DrainRec)) if n else None, n, host_lo, n_hosts,
                                        out.ctypes.data_as(C.POINTER(DrainRec)) if n else None,
                                        spans.ctypes.data_as(C.POINTER(TraceSpan)) if span_cap else None, span_cap, C.byref(ns))
    if rc != 0:
        e = SgnError(rc, ctx.L.sgn_last_error(ctx.h).decode())
        e.out, e.needed = out, ns.value
        raise e
    return out, spans[: ns.value]


def selftest_delay_fold(ctx, recs, piece_ends, host_lo, n_hosts, standing0=None, cap=None):
    """The delay report's kernels on the caller's trace records (TRACE_DTYPE) of hosts [host_lo,
    host_lo + n_hosts), cut into the consecutive pieces recs[piece_ends[i - 1] : piece_ends[i]] (any
    order inside a piece), the carry starting from standing0 unknown entries per host. Returns the
    final Delay. Needs no simulation. An error (SgnError) carries .needed, the row count."""
    recs = np.ascontiguousarray(recs, dtype=TRACE_DTYPE)
    ends = np.ascontiguousarray(piece_ends, dtype=np.uint64)
    s0 = None if standing0 is None else np.ascontiguousarray(standing0, dtype=np.uint32)
    cap = n_hosts if cap is None else cap
    rows = np.zeros(cap, dtype=DELAY_ROW_DTYPE)
    info = DelayInfo()
    n = C.c_uint64()
    rc = ctx.L.sgn_selftest_delay_fold(ctx.h, recs.ctypes.data_as(C.POINTER(TraceRec)) if len(recs) else None,
                                       ptr(ends, C.c_uint64) if len(ends) else None, len(ends), host_lo, n_hosts,
                                       ptr(s0, C.c_uint32) if s0 is not None and len(s0) else None,
                                       rows.ctypes.data_as(C.POINTER(DelayRow)) if cap else None, cap, C.byref(n), C.byref(info))
    if rc != 0:
        e = SgnError(rc, ctx.L.sgn_last_error(ctx.h).decode())
        e.needed = n.value
        raise e
    return Delay(info, rows[: n.value])


def shards_run_until(shards, t_emulated):
    """Runs every shard until the next window would start at or after t_emulated (or the end);
    returns the rounds run (the same on every shard)."""
    d = C.c_uint64()
    _shards_call(shards, "sgn_shards_run_until", t_emulated, C.byref(d))
    return d.value


def shards_snapshot_save(shards):
    """One snapshot handle per shard, all of the same round edge (snaps[i] is owned by shards[i]:
    Context.snapshot_info / snapshot_free apply)."""
    out = (C.c_void_p * len(shards))()
    _shards_call(shards, "sgn_shards_snapshot_save", out)
    return [C.c_void_p(v) for v in out]


def shards_snapshot_restore(shards, snaps):
    arr = (C.c_void_p * len(snaps))(*[s.value if isinstance(s, C.c_void_p) else s for s in snaps])
    _shards_call(shards, "sgn_shards_snapshot_restore", arr)


def snapshot_file_info(path, lib=None):
    """A snapshot file's header (no device, no context): SgnError with rc -2 when the path cannot
    be opened, EFILE when the file is truncated, has another magic or fails its trailer digest."""
    L = lib or load()
    i = SnapshotFileInfo()
    rc = L.sgn_snapshot_file_info_get(os.fsencode(path), C.byref(i))
    if rc != 0:
        raise SgnError(rc, f"sgn_snapshot_file_info_get: {path}")
    return {n: int(getattr(i, n)) for n, _ in i._fields_}


SNAPSHOT_HEADER_BYTES = 288  # snapshot_file.hip FileHeader: the magic and 35 little-endian u64
SNAPSHOT_SECTION_NAMES = ("ctrl", "hrec", "htile", "n_cnt", "maxq", "nextloc", "npeer", "rb_free", "fifo",
                          "fifo_addr", "slab_n", "bucket_slab", "bucket_min", "w_cnt", "codel", "cq_next",
                          "cq_free", "spill", "spill_idx", "drain", "calendar", "handles", "submit_seq",
                          "drain_held", "h_ext", "trace")


def snapshot_file_sections(path):
    """The section table of a snapshot file as [{name, id, bytes, digest, offset}] (offset: of the
    payload in the file; payloads are padded to 16 bytes), read as DESIGN.md lays the file out."""
    n = snapshot_file_info(path)["n_sections"]
    with open(path, "rb") as f:
        f.seek(SNAPSHOT_HEADER_BYTES)
        tab = np.frombuffer(f.read(24 * n), dtype="<u8").reshape(n, 3)
    off = SNAPSHOT_HEADER_BYTES + 24 * n
    out = []
    for i, (sid, nbytes, dig) in enumerate(tab.tolist()):
        name = SNAPSHOT_SECTION_NAMES[i] if i < len(SNAPSHOT_SECTION_NAMES) else str(sid)
        out.append({"name": name, "id": sid, "bytes": nbytes, "digest": dig, "offset": off})
        off += (nbytes + 15) // 16 * 16
    return out


def digest_bytes(buf, lib=None):
    """The section digest of snapshot files over buf (bytes-like, a multiple of 4 bytes), host form."""
    L = lib or load()
    a = np.ascontiguousarray(buf).view(np.uint8).reshape(-1) if isinstance(buf, np.ndarray) else np.frombuffer(bytes(buf), dtype=np.uint8)
    return int(L.sgn_digest_bytes(a.ctypes.data if a.size else None, a.size))


# ------------------------------------------------------------------------------------
# Workload helpers (host side of SimConfig::new: names, IPs, seeds, bandwidth)
# ------------------------------------------------------------------------------------

def host_names(n, prefix="h"):
    width = max(5, len(str(n - 1)))
    return [f"{prefix}{i:0{width}d}" for i in range(n)]


def assign_ips(n, explicit=None, lib=None):
    """assign_ips (core/sim_config.rs:386-407) through libsgn's sgn_assign_ips: hosts in HostId
    order; `explicit` maps host index -> configured IPv4 (int, host byte order); every other
    host gets the next free address from 11.0.0.1 on, skipping .0/.255 and configured ones
    (IpAssignment, network/graph/mod.rs:355-417)."""
    L = lib or load()
    ips = np.zeros(n, dtype=np.uint32)
    flags = np.zeros(n, dtype=np.uint8)
    for i, ip in (explicit or {}).items():
        ips[i] = ip
        flags[i] = 1
    bad = C.c_uint32(0)
    rc = L.sgn_assign_ips(n, ptr(flags, C.c_uint8), ptr(ips, C.c_uint32), C.byref(bad))
    if rc != 0:
        what = "IP address has already been assigned" if rc == -22 else "address space exhausted"
        raise SgnError(rc, f"sgn_assign_ips: host {bad.value}: {what}")
    return ips


def gml_parse(text, lib=None):
    """GML text -> (GraphArrays, [(up_bits|None, down_bits|None) per node]) through libsgn's
    sgn_gml_parse (gml_parser + NetworkGraph::parse, network/graph/mod.rs:28-179)."""
    L = lib or load()
    b = text.encode() if isinstance(text, str) else bytes(text)
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = L.sgn_gml_parse(b, len(b), C.byref(h), err, 512)
    if rc != 0:
        raise SgnError(rc, err.value.decode(errors="replace"))
    try:
        g = Graph()
        L.sgn_gml_graph(h, C.byref(g))
        n, e = g.n_nodes, g.n_edges
        arr = lambda p, k: np.ctypeslib.as_array(p, (k,)).copy() if k else []
        ga = GraphArrays(arr(g.node_id, n), arr(g.edge_src, e), arr(g.edge_dst, e),
                         arr(g.edge_latency_ns, e), arr(g.edge_loss, e), g.directed)
        bws = []
        for i in range(n):
            up, down = C.c_uint64(), C.c_uint64()
            hu, hd = C.c_int32(), C.c_int32()
            L.sgn_gml_node_bandwidth(h, i, C.byref(up), C.byref(hu), C.byref(down), C.byref(hd))
            bws.append((up.value if hu.value else None, down.value if hd.value else None))
    finally:
        L.sgn_gml_free(h)
    return ga, bws


def packet_bytes(src_ip, dst_ip, payload_len, tag=0, lib=None):
    """Packet::display_bytes of one path packet (sgn_packet_bytes)."""
    L = lib or load()
    n = L.sgn_packet_bytes(src_ip, dst_ip, payload_len, tag, None, 0)
    out = np.zeros(n, dtype=np.uint8)
    L.sgn_packet_bytes(src_ip, dst_ip, payload_len, tag, ptr(out, C.c_uint8), n)
    return out.tobytes()


def write_pcaps(trace, host_ips, out_dir, names=None, hosts=None, capture_len=65535, lib=None):
    """Per-host interface captures from trace records (sgn_trace_pcap), one file per host in
    `hosts` (default: every host with a captured packet), laid out like the reference's
    <data_directory>/hosts/<hostname>/eth0.pcap (interface.rs:45-51, namespace.rs:42) when
    names are given (else <out_dir>/h<id>/eth0.pcap). Returns {host: (path, packets)}."""
    L = lib or load()
    tr = np.ascontiguousarray(trace, dtype=TRACE_DTYPE)
    ips = np.ascontiguousarray(host_ips, dtype=np.uint32)
    if hosts is None:
        cap = tr[np.isin(tr["kind"], [TRACE_IF_POP, TRACE_DELIVER, TRACE_LOCAL])]
        hosts = np.unique(cap["host"]).tolist()
    out = {}
    for h in hosts:
        d = os.path.join(out_dir, "hosts", names[h]) if names is not None else os.path.join(out_dir, f"h{h}")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "eth0.pcap")
        n = L.sgn_trace_pcap(tr.ctypes.data_as(C.POINTER(TraceRec)), len(tr), int(h), ptr(ips, C.c_uint32),
                             len(ips), path.encode(), capture_len)
        if n < 0:
            raise SgnError(int(n), f"sgn_trace_pcap host {h}")
        out[int(h)] = (path, int(n))
    return out


class Capture:
    """Per-host interface captures written while the simulation runs (host_options.pcap_enabled,
    interface.rs:45-51): one open writer per captured host at <out_dir>/hosts/<name>/eth0.pcap
    (<out_dir>/h<id>/eth0.pcap without names), each with its own capture length
    (pcap_capture_size). feed() appends one trace_take(); the files end up with the bytes
    write_pcaps gives for the whole trace."""

    def __init__(self, out_dir, host_ips, hosts, capture_sizes=65535, names=None, lib=None):
        self.L = lib or load()
        self.ips = np.ascontiguousarray(host_ips, dtype=np.uint32)
        hosts = [int(h) for h in hosts]
        sizes = [int(capture_sizes)] * len(hosts) if np.ndim(capture_sizes) == 0 else [int(s) for s in capture_sizes]
        if len(sizes) != len(hosts):
            raise ValueError("Capture: one capture size per host")
        self.writers, self.paths, self.packets = {}, {}, {}
        try:
            for h, size in zip(hosts, sizes):
                d = os.path.join(out_dir, "hosts", names[h]) if names is not None else os.path.join(out_dir, f"h{h}")
                os.makedirs(d, exist_ok=True)
                path = os.path.join(d, "eth0.pcap")
                w = C.c_void_p()
                rc = self.L.sgn_pcap_open(os.fsencode(path), size, C.byref(w))
                if rc != 0:
                    raise SgnError(rc, f"sgn_pcap_open {path}")
                self.writers[h], self.paths[h], self.packets[h] = w, path, 0
        except Exception:
            self.close()
            raise

    @property
    def hosts(self):
        return sorted(self.writers)

    def feed(self, records, spans):
        """Appends one take: spans[i] = {host, first, count} over records (trace_take's pair)."""
        recs = np.ascontiguousarray(records, dtype=TRACE_DTYPE)
        for s in spans:
            h, first, count = int(s["host"]), int(s["first"]), int(s["count"])
            w = self.writers.get(h)
            if w is None or count == 0:
                continue
            part = recs[first:first + count]
            n = self.L.sgn_pcap_write_trace(w, part.ctypes.data_as(C.POINTER(TraceRec)), count, h,
                                            ptr(self.ips, C.c_uint32), len(self.ips))
            if n < 0:
                raise SgnError(int(n), f"sgn_pcap_write_trace host {h}")
            self.packets[h] += int(n)

    def close(self):
        """Closes the files; returns {host: (path, packets)} like write_pcaps."""
        err = 0
        for w in self.writers.values():
            err = self.L.sgn_pcap_close(w) or err
        out = {h: (self.paths[h], self.packets[h]) for h in self.writers}
        self.writers = {}
        if err:
            raise SgnError(err, "sgn_pcap_close")
        return out


def run_captured(ctx, capture, step_ns, until=None):
    """Runs ctx (a Context whose trace_hosts are the capture's hosts) to its end, or until the next
    window would start at or after `until`, in steps of step_ns of simulated time: run_until, then
    trace_take, then capture.feed. The trace buffer (trace_enable's capacity) need only hold what
    one step produces. Returns the rounds run."""
    rounds = 0
    while True:
        ws, _, active = ctx.window()
        if not active or (until is not None and ws >= until):
            break
        t = ws + step_ns
        rounds += ctx.run_until(t if until is None else min(t, until))
        capture.feed(*ctx.trace_take())
    capture.feed(*ctx.trace_take())  # (records produced before the call, if any)
    return rounds


class Samples:
    """The samples of a run: .infos (SAMPLE_INFO_DTYPE, one per sample, in order) and .rows
    (SAMPLE_ROW_DTYPE, ordered by sample, then host); infos[k]'s rows are rows[first_row :
    first_row + rows]. A host that did not change in an interval has no row there."""

    def __init__(self, rows=None, infos=None):
        self.rows = np.zeros(0, SAMPLE_ROW_DTYPE) if rows is None else np.ascontiguousarray(rows, dtype=SAMPLE_ROW_DTYPE)
        self.infos = np.zeros(0, SAMPLE_INFO_DTYPE) if infos is None else np.ascontiguousarray(infos, dtype=SAMPLE_INFO_DTYPE)
        if int(self.infos["rows"].sum()) != len(self.rows):
            raise ValueError("Samples: the infos' row counts do not add up to the rows")

    @classmethod
    def from_takes(cls, takes):
        """One Samples from the (rows, infos) pairs of successive sample_take() calls: first_row
        counts from the first take's first row."""
        rows = [np.zeros(0, SAMPLE_ROW_DTYPE)] + [r for r, _ in takes]
        infos = [np.zeros(0, SAMPLE_INFO_DTYPE)]
        base = 0
        for r, i in takes:
            i = i.copy()
            i["first_row"] += base
            infos.append(i)
            base += len(r)
        return cls(np.concatenate(rows), np.concatenate(infos))

    def __len__(self):
        return len(self.infos)

    def dense(self, field, n_hosts):
        """[samples, n_hosts] u64: the field's delta of every host in every interval (0 where the
        host has no row)."""
        out = np.zeros((len(self.infos), n_hosts), dtype=np.uint64)
        k = np.repeat(np.arange(len(self.infos)), self.infos["rows"].astype(np.int64))
        out[k, self.rows["host"]] = self.rows[field]
        return out

    def cumulative(self, field, n_hosts):
        """[samples, n_hosts] u64: the field's growth since the baseline, at every sample."""
        return np.cumsum(self.dense(field, n_hosts), axis=0, dtype=np.uint64)


class Backlog:
    """One backlog report (Context.backlog): .info, a dict of sgn_backlog_info (total: the eight sums
    in BACKLOG_TOTALS order; .totals: the same by name), and .rows (BACKLOG_ROW_DTYPE, ascending by
    host; empty for the totals-only form)."""

    def __init__(self, info, rows=None):
        self.info = {f[0]: ([int(v) for v in getattr(info, f[0])] if len(f) > 2 else int(getattr(info, f[0])))
                     for f in _BACKLOG_INFO if not f[0].startswith("pad")}
        self.rows = np.zeros(0, BACKLOG_ROW_DTYPE) if rows is None else np.ascontiguousarray(rows, dtype=BACKLOG_ROW_DTYPE)

    @property
    def totals(self):
        return dict(zip(BACKLOG_TOTALS, self.info["total"]))

    def dense(self, field, n_hosts=None):
        """The field of every host, indexed by HostId, zeros where no row exists (also for the two
        times that are SGN_EMUTIME_INVALID in a row without them). n_hosts: the array's length —
        default the owned hosts, which covers an unsharded context; a shard's rows need the
        simulation's host count."""
        n = int(self.info["hosts"]) if n_hosts is None else int(n_hosts)
        out = np.zeros(n, dtype=BACKLOG_ROW_DTYPE.fields[field][0])
        v = self.rows[field].copy()
        if field in ("router_oldest", "inflight_earliest"):
            v[v == EMUTIME_INVALID] = 0
        out[self.rows["host"]] = v
        return out


class Delay:
    """One router delay report (Context.delay): .info, a dict of sgn_delay_info (total: the six sums in
    DELAY_TOTALS order; .totals: the same by name; hist_delivered / hist_dropped: DELAY_BINS counts),
    and .rows (DELAY_ROW_DTYPE, ascending by host; empty for the totals-only form)."""

    def __init__(self, info, rows=None):
        self.info = {f[0]: ([int(v) for v in getattr(info, f[0])] if len(f) > 2 else int(getattr(info, f[0])))
                     for f in _DELAY_INFO if not f[0].startswith("pad")}
        self.rows = np.zeros(0, DELAY_ROW_DTYPE) if rows is None else np.ascontiguousarray(rows, dtype=DELAY_ROW_DTYPE)

    @property
    def totals(self):
        return dict(zip(DELAY_TOTALS, self.info["total"]))

    def quantile(self, q, dropped=False):
        """The upper edge, in ns, of the histogram bin that holds the q-th (0 < q <= 1) matched packet
        in delay order: delivered packets, or CoDel-dropped ones. None when no packet was matched."""
        hist = self.info["hist_dropped" if dropped else "hist_delivered"]
        n = sum(hist)
        if n == 0:
            return None
        want = min(n, max(1, int(np.ceil(q * n))))  # (at least the first packet)
        seen = 0
        for edge, c in zip(delay_bin_edges(), hist):
            seen += c
            if seen >= want:
                return edge
        return delay_bin_edges()[-1]


def run_delays(ctx, step_ns, until=None):
    """Runs ctx (a traced Context with delay_enable() done) to its end, or until the next window would
    start at or after `until`, in steps of step_ns of simulated time: run_until, then delay_fold. The
    trace buffer need only hold what one step produces. Returns the final Delay."""
    while True:
        ws, _, active = ctx.window()
        if not active or (until is not None and ws >= until):
            break
        t = ws + step_ns
        ctx.run_until(t if until is None else min(t, until))
        ctx.delay_fold()
    ctx.delay_fold()  # (records produced before the call, if any)
    return ctx.delay()


def run_sampled(ctx_or_shards, interval_ns, until=None, backlog=False):
    """Runs a Context — or this process's shards, as shards_run_until takes them — to the end, or
    until the next window would start at or after `until`, sampling at every multiple of
    interval_ns of simulated time at which anything was left to run: run_until the next multiple
    above the window start, then sample() on every context (sample_enable first; its row capacity
    need only hold a few samples: the rows are taken when they pass half of it, and at the end).
    Returns the Samples of the context, or a list of them, one per shard.
    backlog=True: after each sample the backlog totals are taken too (Context.backlog(rows=False))
    and every returned Samples carries backlog_total[samples, 8] (BACKLOG_TOTALS order; summed over
    the shards) and backlog_max_router[samples] (the largest CoDel queue; the shards' maximum)."""
    many = isinstance(ctx_or_shards, (list, tuple))
    ctxs = list(ctx_or_shards) if many else [ctx_or_shards]
    takes = [[] for _ in ctxs]
    bl_total, bl_max = [], []
    while True:
        ws, _, active = ctxs[0].window()
        if not active or (until is not None and ws >= until):
            break
        t = SIMULATION_START + ((ws - SIMULATION_START) // interval_ns + 1) * interval_ns
        t = t if until is None else min(t, until)
        if many:
            shards_run_until(ctxs, t)
        else:
            ctxs[0].run_until(t)
        for c, tk in zip(ctxs, takes):
            try:
                c.sample()
            except SgnError as e:
                if e.rc != EOVERFLOW or c.sample_pending()[0] == 0:
                    raise
                tk.append(c.sample_take())
                c.sample()
            if 2 * c.sample_pending()[0] > c.sample_capacity:
                tk.append(c.sample_take())
        if backlog:  # the totals-only form on every context, after the sample
            infos = [c.backlog(rows=False).info for c in ctxs]
            bl_total.append(np.sum([i["total"] for i in infos], axis=0, dtype=np.uint64))
            bl_max.append(max(i["max_router_packets"] for i in infos))
    for c, tk in zip(ctxs, takes):
        tk.append(c.sample_take())
    out = [Samples.from_takes(tk) for tk in takes]
    if backlog:
        for s in out:
            s.backlog_total = np.array(bl_total, dtype=np.uint64).reshape(len(bl_total), 8)
            s.backlog_max_router = np.array(bl_max, dtype=np.uint64)
    return out if many else out[0]


def derive_seeds(sim_seed, names, lib=None):
    L = lib or load()
    arr = (C.c_char_p * len(names))(*[s.encode() for s in names])
    out = np.zeros(len(names), dtype=np.uint64)
    rc = L.sgn_derive_host_seeds(sim_seed, arr, len(names), ptr(out, C.c_uint64))
    if rc != 0:
        raise SgnError(rc, "sgn_derive_host_seeds")
    return out


def random_graph(V, mean_degree=6, seed=42, lat_lo_us=1000, lat_hi_us=50000,
                 loss_frac=0.2, loss_hi=0.02):
    """Config B graph: undirected spanning tree + random extra edges to the mean degree,
    one self-loop per node (1 ms, loss 0). Loss values are rounded to 6 decimals as they
    would be printed into GML, then parsed as f32."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    perm = rng.permutation(V)
    for i in range(1, V):
        j = int(rng.integers(0, i))
        src.append(int(perm[i]))
        dst.append(int(perm[j]))
    extra = max(0, V * mean_degree // 2 - (V - 1))
    seen = set((min(a, b), max(a, b)) for a, b in zip(src, dst))
    while extra > 0:
        a, b = (int(x) for x in rng.integers(0, V, 2))
        if a == b or (min(a, b), max(a, b)) in seen:
            continue
        seen.add((min(a, b), max(a, b)))
        src.append(a)
        dst.append(b)
        extra -= 1
    E = len(src)
    lat = rng.integers(lat_lo_us, lat_hi_us + 1, E).astype(np.uint64) * 1000
    lossy = rng.random(E) < loss_frac
    loss = np.where(lossy, np.round(rng.uniform(1e-4, loss_hi, E), 6), 0.0)
    loss = np.array([np.float32(float(f"{x:.6f}")) for x in loss], dtype=np.float32)
    src += list(range(V))
    dst += list(range(V))
    lat = np.concatenate([lat, np.full(V, 1_000_000, dtype=np.uint64)])
    loss = np.concatenate([loss, np.zeros(V, dtype=np.float32)])
    return GraphArrays(np.arange(V), src, dst, lat, loss, directed=False)


def tor_graph(V, seed=42):
    """Config C graph: complete graph over V 'city' nodes. Latency = 1 ms + a distance term
    (5-150 ms) from random points on a sphere; loss 0-0.5 %; self-loop 1 ms."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1, 1, V)
    t = rng.uniform(0, 2 * np.pi, V)
    r = np.sqrt(1 - z * z)
    P = np.stack([r * np.cos(t), r * np.sin(t), z], 1)
    iu, ju = np.triu_indices(V, 1)
    ang = np.arccos(np.clip((P[iu] * P[ju]).sum(1), -1, 1)) / np.pi
    lat_us = (1000 + 5000 + ang * 145000).astype(np.uint64)
    loss = np.round(rng.uniform(0, 0.005, len(iu)), 6).astype(np.float32)
    src = np.concatenate([iu, np.arange(V)])
    dst = np.concatenate([ju, np.arange(V)])
    lat = np.concatenate([lat_us * 1000, np.full(V, 1_000_000, dtype=np.uint64)])
    loss = np.concatenate([loss, np.zeros(V, dtype=np.float32)])
    return GraphArrays(np.arange(V), src, dst, lat, loss, directed=False)


def bandwidth_classes(n, seed=3, classes=(10_000_000, 100_000_000, 1_000_000_000)):
    rng = np.random.default_rng(seed)
    return np.array(classes, dtype=np.uint64)[rng.integers(0, len(classes), n)]


def zipf_nodes(n_hosts, V, seed=5, s=1.0):
    """Host -> node with a Zipf(s) node popularity (config C)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, V + 1) ** s
    w /= w.sum()
    order = rng.permutation(V)
    return order[rng.choice(V, size=n_hosts, p=w)].astype(np.uint32)
