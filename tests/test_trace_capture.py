"""A trace of chosen hosts streamed into per-host captures, CPU side (no GPU call):

* the new entry points (sgn_trace_hosts, sgn_trace_pending, sgn_trace_take, sgn_pcap_write_trace)
  are exported, refuse null arguments, and leave the ABI version alone (they are additive);
* sgn_pcap_write_trace fed one host's records in pieces writes the bytes sgn_trace_pcap writes from
  the whole trace (the oracle's external-application trace: unknown addresses, loopback, TCP
  sizes), at the default capture length and at 40 bytes;
* shadow_config.sim_setup reports the hosts with pcap_enabled after host_option_defaults and the
  per-host overrides, with their capture sizes.
The GPU side (the host filter, the ordered takes, snapshots, shards, the capture loop) is in
tests/test_gpu_trace_capture.py.
"""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import sgn
import shadow_config as sc
from test_pcap import GOLD_HEADER

EINVAL = -22
NAMES = ("sgn_trace_hosts", "sgn_trace_pending", "sgn_trace_take", "sgn_trace_take_timing_get", "sgn_pcap_write_trace")
CAPTURED = (sgn.TRACE_IF_POP, sgn.TRACE_DELIVER, sgn.TRACE_LOCAL)


def test_library_exports_trace_capture(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10
    assert C.sizeof(sgn.TraceSpan) == 24 and C.sizeof(sgn.TraceRec) == 56


def test_null_arguments_are_refused(lib, tmp_path):
    n, ns = C.c_uint64(7), C.c_uint64(7)
    hosts = np.array([1, 2], dtype=np.uint32)
    rec = np.zeros(1, dtype=sgn.TRACE_DTYPE)
    ips = np.array([1, 2], dtype=np.uint32)
    assert lib.sgn_trace_hosts(None, sgn.ptr(hosts, C.c_uint32), 2) == EINVAL
    assert lib.sgn_trace_pending(None, C.byref(n)) == EINVAL and n.value == 0
    n.value = 7
    assert lib.sgn_trace_take(None, rec.ctypes.data_as(C.POINTER(sgn.TraceRec)), 1, C.byref(n), None, 0, C.byref(ns)) == EINVAL
    assert n.value == 0 and ns.value == 0
    assert lib.sgn_trace_take_timing_get(None, None) == EINVAL
    assert lib.sgn_pcap_write_trace(None, rec.ctypes.data_as(C.POINTER(sgn.TraceRec)), 1, 0, sgn.ptr(ips, C.c_uint32), 2) == EINVAL
    w = C.c_void_p()
    assert lib.sgn_pcap_open(str(tmp_path / "w.pcap").encode(), 65535, C.byref(w)) == 0
    rp, ip = rec.ctypes.data_as(C.POINTER(sgn.TraceRec)), sgn.ptr(ips, C.c_uint32)
    assert lib.sgn_pcap_write_trace(w, None, 1, 0, ip, 2) == EINVAL       # records missing
    assert lib.sgn_pcap_write_trace(w, rp, 1, 0, None, 2) == EINVAL       # addresses missing
    assert lib.sgn_pcap_write_trace(w, rp, 1, 2, ip, 2) == EINVAL         # host outside the table
    assert lib.sgn_pcap_write_trace(w, None, 0, 0, ip, 2) == 0            # nothing to write
    assert lib.sgn_pcap_close(w) == 0
    assert (tmp_path / "w.pcap").read_bytes() == GOLD_HEADER


@pytest.fixture(scope="module")
def external_trace(oracle):
    from external_common import datagrams, drive, external_world
    g, used, hosts, cfg, tr = external_world()
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)
    drive([o], datagrams(hosts))
    t = o.trace()
    return t[np.lexsort((t["seq"], t["host"]))], hosts


def _busiest(t):
    cap = t[np.isin(t["kind"], CAPTURED)]
    h = int(np.bincount(cap["host"]).argmax())
    return h, t[t["host"] == h]


@pytest.mark.parametrize("capture_len", [65535, 40])
def test_streaming_writer_matches_whole_trace(lib, external_trace, tmp_path, capture_len):
    t, hosts = external_trace
    h, mine = _busiest(t)
    assert np.isin(mine["kind"], CAPTURED).sum() > 30 and set(CAPTURED) <= set(mine["kind"].tolist())
    ips = np.ascontiguousarray(hosts.ip, dtype=np.uint32)
    whole = tmp_path / "whole.pcap"
    tt = np.ascontiguousarray(t)
    n = lib.sgn_trace_pcap(tt.ctypes.data_as(C.POINTER(sgn.TraceRec)), len(tt), h, sgn.ptr(ips, C.c_uint32), len(ips),
                           str(whole).encode(), capture_len)
    assert n == np.isin(mine["kind"], CAPTURED).sum()
    # the host's records in seq order, in three uneven pieces (the first cut inside a run of
    # captured records), each handed over with other hosts' records around it
    cuts = [0, len(mine) // 5, len(mine) // 5 + 1 + len(mine) // 2, len(mine)]
    other = t[t["host"] != h][:50]
    w = C.c_void_p()
    path = tmp_path / "pieces.pcap"
    assert lib.sgn_pcap_open(str(path).encode(), capture_len, C.byref(w)) == 0
    got = 0
    for a, b in zip(cuts, cuts[1:]):
        part = np.ascontiguousarray(np.concatenate([other[:7], mine[a:b], other[7:]]))
        k = lib.sgn_pcap_write_trace(w, part.ctypes.data_as(C.POINTER(sgn.TraceRec)), len(part), h,
                                     sgn.ptr(ips, C.c_uint32), len(ips))
        assert k >= 0
        got += k
    assert lib.sgn_pcap_close(w) == 0
    assert got == n
    data = path.read_bytes()
    assert data == whole.read_bytes()
    head = bytearray(GOLD_HEADER)
    head[16:20] = capture_len.to_bytes(4, "little")  # the global header's snaplen
    assert data[:24] == bytes(head) and len(data) > 24
    if capture_len == 40:  # every packet is at least 28 bytes of headers; longer ones are cut at 40
        i, cut = 24, 0
        while i < len(data):
            cap, ln = int.from_bytes(data[i + 8:i + 12], "little"), int.from_bytes(data[i + 12:i + 16], "little")
            assert cap == min(ln, 40)
            cut += ln > 40
            i += 16 + cap
        assert cut > 0


def test_capture_class_feeds_spans(lib, external_trace, tmp_path):
    """sgn.Capture over two hosts with different capture lengths, fed the trace in two pieces as
    (records, spans) pairs, against write_pcaps of the whole trace."""
    t, hosts = external_trace
    names = sgn.host_names(hosts.n)
    cap = t[np.isin(t["kind"], CAPTURED)]
    busy = np.argsort(np.bincount(cap["host"], minlength=hosts.n))[-2:].tolist()
    sizes = [65535, 96]
    want = {}
    for h, s in zip(busy, sizes):
        want.update(sgn.write_pcaps(t, hosts.ip, tmp_path / "whole", names=names, hosts=[h], capture_len=s))

    def spans_of(recs):  # what sgn_trace_take returns for records sorted by (host, seq)
        hs, first, count = np.unique(recs["host"], return_index=True, return_counts=True)
        sp = np.zeros(len(hs), dtype=sgn.SPAN_DTYPE)
        sp["host"], sp["first"], sp["count"] = hs, first, count
        return sp

    c = sgn.Capture(tmp_path / "stream", hosts.ip, busy, sizes, names=names)
    assert c.hosts == sorted(busy)
    # a take holds a prefix of every host's remaining records: split each host's records in two
    first = np.zeros(len(t), dtype=bool)
    for h in np.unique(t["host"]):
        idx = np.nonzero(t["host"] == h)[0]
        first[idx[: len(idx) // 3]] = True
    for piece in (t[first], t[~first]):
        c.feed(piece, spans_of(piece))
    got = c.close()
    assert got.keys() == want.keys()
    for h in want:
        assert got[h][0].endswith(f"hosts/{names[h]}/eth0.pcap")
        assert got[h][1] == want[h][1] > 0
        assert open(got[h][0], "rb").read() == open(want[h][0], "rb").read(), h


PCAP_YAML = """
general:
  stop_time: 10 s
network:
  graph:
    type: 1_gbit_switch
host_option_defaults:
  pcap_enabled: true
hosts:
  alpha:
    network_node_id: 0
    processes:
    - path: /bin/true
  bravo:
    network_node_id: 0
    host_options:
      pcap_enabled: false
    processes:
    - path: /bin/true
  charlie:
    network_node_id: 0
    host_options:
      pcap_capture_size: 96 B
    processes:
    - path: /bin/true
  delta:
    network_node_id: 0
    processes:
    - path: /bin/true
"""


def test_front_end_reports_pcap_hosts():
    setup = sc.sim_setup(sc.load(text=PCAP_YAML))
    assert setup.names == ["alpha", "bravo", "charlie", "delta"]
    assert setup.pcap_hosts == [0, 2, 3]
    assert setup.pcap_capture_size == [65535, 96, 65535]
    # the default is off: a file that never mentions pcap captures nothing
    off = sc.sim_setup(sc.load(text=PCAP_YAML.replace("host_option_defaults:\n  pcap_enabled: true\n", "")
                               .replace("      pcap_enabled: false\n", "      pcap_enabled: true\n")))
    assert off.pcap_hosts == [1] and off.pcap_capture_size == [65535]
