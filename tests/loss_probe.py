"""Loss-draw boundary probes: chosen draws of chosen hosts placed exactly on the drop threshold.

Worker::send_packet (core/worker.rs:363-371) drops a packet iff `chance >= reliability`, with
chance = (x >> 11) * 2^-53 for the source host's next xoshiro256++ output x and reliability =
(f64)(1.0f - loss). With T = (u64)(reliability * 2^53) that is (x >> 11) >= T, or x >= Tx with
Tx = T << 11. For reliability >= 2^-8, 1.0f - loss is a multiple of 2^-24, so the low word of
Tx is 0, its high word Th is a multiple of 256 and the decision is hi32(x) >= Th. Conversely
every Th = k << 8 (0 < k < 2^24) is the threshold of the exact f32 loss 1 - k / 2^24.

This module restates SplitMix64 seeding and xoshiro256++ in plain numpy (independent of libsgn
and of the oracle), searches seeds for a draw whose high word is a multiple of 256 (a
threshold itself) or one below a multiple, and builds a scenario in which every packet a probe
host sends meets the loss that puts Th on that draw: a complete DIRECTED graph whose arc a -> b
loses L[a] whatever b (self-loop included), every arc 5 ms (self-loops 1 ms), so the direct arc
is the unique shortest path and a one-arc path keeps the arc's loss unchanged.

Probe classes (Th >= SCREEN_TH takes the TGEN kernel's carry-less screen, lower Th the exact
eight / four / one-draw tests; "carry": the add of the output's low words carries into hi32):
    A  hi32(x) == Th      carry     drop   (the carry-less word is Th - 1)
    B  hi32(x) == Th      no carry  drop
    C  hi32(x) == Th - 1  no carry  keep   (the carry-less word is Th - 1: the batch is redone)
    D  hi32(x) == Th - 1  carry     keep   (the carry-less word is Th - 2: the screen passes)
    E  hi32(x) == Th      any       drop   Th < SCREEN_TH
    F  hi32(x) == Th - 1  any       keep   Th < SCREEN_TH
hi32(x) == Th makes x >= Tx whatever x's low word, so these tell `>=` from `>` only on the high
words. Two more classes, on any Th, put the whole draw on the threshold:
    G  x == Tx                      drop   (x's low 40 bits are 0: `x > Tx` keeps it)
    H  x >> 11 == T, x > Tx         drop   (bits 11..39 are 0: `(x >> 11) > T` keeps it)
"""
import collections

import numpy as np

SCREEN_TH = 0xF8000000   # lowest screened threshold: loss exactly 1/32
WINDOW = (64, 320)       # draw indices the probes lie in: every probe host sends more packets
CLASSES = "ABCDEF"
U64 = np.uint64

Probe = collections.namedtuple("Probe", "cls seed index Th loss drop x carry")


def _u(v):
    return U64(v & 0xFFFFFFFFFFFFFFFF)


def _rotl(x, k):
    return (x << U64(k)) | (x >> U64(64 - k))


def mix64(z):
    """SplitMix64's output function on a uint64 array."""
    z = (z ^ (z >> U64(30))) * _u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * _u(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def seed_state(seeds):
    """rand_core SeedableRng::seed_from_u64 for Xoshiro256PlusPlus: four SplitMix64 outputs.
    seeds: uint64 array (n,) -> state (4, n)."""
    st = np.array(seeds, dtype=U64, ndmin=1)
    out = []
    with np.errstate(over="ignore"):
        for _ in range(4):
            st = st + _u(0x9E3779B97F4A7C15)
            out.append(mix64(st))
    return np.stack(out)


def _step(s):
    s0, s1, s2, s3 = s
    t = s1 << U64(17)
    s2 = s2 ^ s0
    s3 = s3 ^ s1
    s1 = s1 ^ s2
    s0 = s0 ^ s3
    s2 = s2 ^ t
    s3 = _rotl(s3, 45)
    return [s0, s1, s2, s3]


def draws(seeds, lo, hi):
    """Draws lo..hi-1 of every seed's stream: (x, carry), both (n, hi - lo). x is next_u64's
    output rotl(s0 + s3, 23) + s0; carry says whether hi32(x) is one more than the carry-less
    word hi32(rotl(s0 + s3, 23)) + hi32(s0) (mod 2^32)."""
    s = list(seed_state(seeds))
    n = len(s[0])
    x = np.empty((n, hi - lo), dtype=U64)
    carry = np.empty((n, hi - lo), dtype=bool)
    with np.errstate(over="ignore"):
        for i in range(hi):
            if i >= lo:
                r = _rotl(s[0] + s[3], 23)
                xi = r + s[0]
                nc = ((r >> U64(32)) + (s[0] >> U64(32))) & U64(0xFFFFFFFF)
                x[:, i - lo] = xi
                carry[:, i - lo] = (xi >> U64(32)) != nc
            s = _step(s)
    return x, carry


def state_after(seeds, counts):
    """The xoshiro256++ state (n, 4) of every seed after counts[i] draws."""
    s = list(seed_state(seeds))
    counts = np.asarray(counts, dtype=np.int64)
    out = np.stack(s, axis=1)
    for i in range(int(counts.max(initial=0))):
        s = _step(s)
        done = counts == i + 1
        if done.any():
            out[done] = np.stack(s, axis=1)[done]
    return out


def loss_of(Th):
    """The f32 loss whose threshold's high word is Th = k << 8: 1 - k / 2^24, exact."""
    assert 0 < Th < 1 << 32 and Th % 256 == 0, hex(Th)
    loss = np.float32(1.0 - (Th >> 8) / 2.0 ** 24)
    assert th_of(loss) == Th, (hex(Th), loss)
    return loss


def th_of(loss):
    """hi32 of Tx = T << 11, T = (u64)((f64)(1.0f - loss) * 2^53), for an f32 loss."""
    rel = np.float32(1.0) - np.float32(loss)
    T = int(np.float64(rel) * 2.0 ** 53)
    return (T << 11) >> 32


def classify(x, carry):
    """The class a draw would probe (None: its high word is not on a threshold) and that Th."""
    h = int(x) >> 32
    if h % 256 == 0 and h > 0:
        Th, at = h, True
    elif h % 256 == 255 and h != 0xFFFFFFFF:
        Th, at = h + 1, False
    else:
        return None, 0
    if Th >= SCREEN_TH:
        return ("A" if carry else "B") if at else ("D" if carry else "C"), Th
    return "E" if at else "F", Th


def make_probe(seed, index, x, carry):
    cls, Th = classify(x, carry)
    assert cls is not None
    drop = cls in "ABE"
    if drop and int(x) & 0xFFFFFFF800 == 0:
        cls = "H" if int(x) & 0x7FF else "G"
        assert (int(x) >> 11 == (Th << 32) >> 11) and (cls == "H" or int(x) == Th << 32)
    assert drop == ((int(x) >> 32) >= Th) == (int(x) >= Th << 32)
    return Probe(cls, int(seed), int(index), Th, loss_of(Th), drop, int(x), bool(carry))


_cands = None


def candidates():
    """Every draw in WINDOW of seeds 1..2^15 that lies on a threshold, by class: lists of
    (seed, index, x, carry) in seed order."""
    global _cands
    if _cands is not None:
        return _cands
    seeds = np.arange(1, (1 << 15) + 1, dtype=U64)
    x, carry = draws(seeds, *WINDOW)
    low = (x >> U64(32)) & U64(0xFF)
    si, di = np.nonzero((low == U64(0)) | (low == U64(0xFF)))
    out = {c: [] for c in CLASSES}
    for s, d in zip(si, di):
        cls, _ = classify(x[s, d], carry[s, d])
        if cls is not None:
            out[cls].append((int(seeds[s]), WINDOW[0] + int(d), int(x[s, d]), bool(carry[s, d])))
    _cands = out
    return out


def search(cls, count, taken=()):
    """count probes of a class on distinct seeds (none in `taken`), their draw indices spread
    over index % 8 and over WINDOW; three in four of classes E and F have Th <= 2^31 (a path
    losing at least half of its packets), which the fixed probes at the cut have not."""
    cand = candidates()[cls]
    used = set(taken)
    lo, hi = WINDOW
    probes = []
    for r in range(count):
        w0 = lo + (hi - lo) * r // count
        w1 = lo + (hi - lo) * (r + 1) // count

        def ok(c, window, residue):
            if c[0] in used:
                return False
            if cls in "EF":
                _, Th = classify(c[2], c[3])
                if (Th <= 1 << 31) != (r % 4 != 3):
                    return False
            return (not window or w0 <= c[1] < w1) and (not residue or c[1] % 8 == r % 8)
        pick = next((c for c in cand if ok(c, True, True)), None) or \
            next((c for c in cand if ok(c, False, True)), None)
        assert pick is not None, (cls, r)
        used.add(pick[0])
        probes.append(make_probe(*pick))
    return probes


# Thresholds at the cut between the screen and the exact form: Th = SCREEN_TH (loss exactly
# 1/32) and the next one below. A draw with one given high word turns up once in 2^32, so these
# seeds come from an exhaustive offline search (seeds 1.., draws in WINDOW); fixed_probes()
# recomputes every one of them from the numpy stream.
FIXED = (
    # (seed, index, hi32(x))
    (108819870, 185, 0xF8000000),  # A: Th = SCREEN_TH
    (20665037, 295, 0xF8000000),   # B
    (32474112, 125, 0xF7FFFFFF),   # C
    (112682593, 203, 0xF7FFFFFF),  # D
    (892350, 299, 0xF7FFFF00),     # E: Th = SCREEN_TH - 256, the highest in the exact form
    (59255300, 157, 0xF7FFFF00),   # E
    (70198082, 144, 0xF7FFFEFF),   # F
)


# Draws that equal their threshold beyond the high word (classes G and H: one draw in 2^40 and
# one in 2^29), from the same kind of search.
FIXED_EXACT = (
    # (seed, index, x)
    (3677696777, 313, 0x58F70F0000000000),  # G, a path losing 65 %
    (3940249775, 156, 0x3016CD0000000000),  # G, a path losing 81 %
    (3754122437, 115, 0xF9674B0000000000),  # G, screened
    (9317449, 178, 0xF9743B0000000387),    # H, screened
    (140268921, 158, 0xFED3C100000004A3),  # H, screened
    (797242, 208, 0x878D690000000594),     # H
    (5254586, 292, 0x1948F00000000434),    # H, a path losing 90 %
    (9330897, 78, 0xC5D5E700000007C8),     # H
)


def fixed_probes():
    out = []
    for seed, index, want in FIXED + FIXED_EXACT:
        x, carry = draws(np.array([seed], dtype=U64), index, index + 1)
        exact = want >= 1 << 32
        assert int(x[0, 0]) >> (0 if exact else 32) == want, (seed, index, hex(int(x[0, 0])))
        p = make_probe(seed, index, x[0, 0], carry[0, 0])
        assert WINDOW[0] <= index < WINDOW[1]
        assert p.cls in "GH" if exact else p.Th in (SCREEN_TH, SCREEN_TH - 256)
        out.append(p)
    return out


_sets = {}


def probe_set(per_class=8):
    """per_class probes of every class A-F and the fixed ones at the cut, on distinct seeds."""
    if per_class not in _sets:
        probes = fixed_probes()
        for cls in CLASSES:
            probes += search(cls, per_class, taken=[p.seed for p in probes])
        assert len({p.seed for p in probes}) == len(probes)
        _sets[per_class] = tuple(probes)
    return list(_sets[per_class])


def auto_ips(n):
    """Automatic addresses in HostId order: 11.0.0.1 on, skipping .0 and .255
    (network/graph/mod.rs:359-417)."""
    ips, a = [], (11 << 24) + 1
    while len(ips) < n:
        if a & 0xFF not in (0, 255):
            ips.append(a)
        a += 1
    return np.array(ips, dtype=np.uint32)


def plain_seeds(n, salt=0xC0FFEE):
    """Ordinary seeds for the hosts that are no probes."""
    with np.errstate(over="ignore"):
        return mix64((np.arange(n, dtype=U64) + U64(1)) * _u(0x9E3779B97F4A7C15) ^ U64(salt))


def star_loss_graph(losses):
    """Complete directed graph on len(losses) nodes: arc a -> b loses losses[a] for every b
    (the self-loop too); 5 ms arcs, 1 ms self-loops."""
    import sgn
    V = len(losses)
    a, b = np.divmod(np.arange(V * V), V)
    lat = np.where(a == b, 1_000_000, 5_000_000).astype(np.uint64)
    return sgn.GraphArrays(np.arange(V), a, b, lat, np.asarray(losses, dtype=np.float32)[a], True)


def hosts_on(V, per_node, seeds0, bw0, bw_rest):
    """Host v < V sits on node v (seed seeds0[v], bandwidths bw0 = (up, down)); per_node more
    hosts follow on every node with plain seeds and bandwidths bw_rest."""
    import sgn
    n = V * (1 + per_node)
    node = np.concatenate([np.arange(V), np.repeat(np.arange(V), per_node)])
    seed = np.concatenate([np.asarray(seeds0, dtype=U64), plain_seeds(V * per_node)])
    up = np.where(np.arange(n) < V, bw0[0], bw_rest[0]).astype(np.uint64)
    down = np.where(np.arange(n) < V, bw0[1], bw_rest[1]).astype(np.uint64)
    assert (up != down).all()
    return sgn.HostArrays(auto_ips(n), node, up, down, seed)


STOP_NS = 600_000_000


def tgen_scenario(probes, clients_per_node=3):
    """TGEN probes: node v holds probe host v, a 1 Gbit/s server whose refills admit dozens of
    packets per send (so most of its draws fall into eight-draw batches), and a few 100 Mbit/s
    clients; 600 ms."""
    import sgn
    V = len(probes)
    g = star_loss_graph([p.loss for p in probes])
    hosts = hosts_on(V, clients_per_node, [p.seed for p in probes],
                     (1_000_000_000, 900_000_000), (90_000_000, 100_000_000))
    cfg = sgn.make_config(STOP_NS, out_fifo_cap=64, codel_cap=4096, event_capacity=1 << 20)
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, period_ns=20_000_000, period_jitter_ns=20_000_000,
                          start_jitter_ns=20_000_000, servers=np.arange(V),
                          file_bytes=(50 * 1024, 300 * 1024, 1024 * 1024))
    return g, np.arange(V), hosts, cfg, tr


def periodic_scenario(probes):
    """PERIODIC probes: one probe host per node and nothing else, a datagram every
    millisecond; 600 ms."""
    import sgn
    V = len(probes)
    g = star_loss_graph([p.loss for p in probes])
    hosts = hosts_on(V, 0, [p.seed for p in probes], (100_000_000, 90_000_000), (0, 1))
    cfg = sgn.make_config(STOP_NS, out_fifo_cap=64, codel_cap=4096, event_capacity=1 << 20)
    tr = sgn.make_traffic(period_ns=1_000_000, start_jitter_ns=3_000_000, payload_len=1024)
    return g, np.arange(V), hosts, cfg, tr


END_LOSSES = np.array([0.0, 2.0 ** -24, 1 / 32, np.nextafter(np.float32(1 / 32), np.float32(1)),
                       0.5, 1 - 2.0 ** -24, 1.0], dtype=np.float32)
END_LOSS_ALL = 6  # the node whose paths lose everything
END_CASES = {"periodic-1024": ("periodic", 1024), "periodic-0": ("periodic", 0),
             "tgen-64": ("tgen", 64), "tgen-0": ("tgen", 0)}


def ends_scenario(case):
    """The ends of the loss range on direct paths (routes_build(..., shortest=False): the
    table holds the arc's own value). Node v loses END_LOSSES[v]; host v is node v's server
    under TGEN; three more hosts per node."""
    import sgn
    kind, payload = END_CASES[case]
    V = len(END_LOSSES)
    g = star_loss_graph(END_LOSSES)
    hosts = hosts_on(V, 3, plain_seeds(V, salt=0xE2D5), (1_000_000_000, 900_000_000),
                     (90_000_000, 100_000_000))
    cfg = sgn.make_config(300_000_000, out_fifo_cap=64, codel_cap=4096, event_capacity=1 << 20)
    if kind == "periodic":
        tr = sgn.make_traffic(period_ns=1_000_000, start_jitter_ns=3_000_000, payload_len=payload)
    else:
        tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, period_ns=20_000_000, period_jitter_ns=20_000_000,
                              start_jitter_ns=20_000_000, servers=np.arange(V), req_payload=payload,
                              file_bytes=(50 * 1024, 300 * 1024, 1024 * 1024))
    return g, np.arange(V), hosts, cfg, tr


def check_ends(case, sim, hosts, trace=None):
    """What a run of ends_scenario(case) must show whoever computed it (sim: the oracle's Sim
    or a libsgn Context, after run()): nothing with a payload leaves the node that loses
    everything, an empty payload is never dropped, and every send draws — the host's final
    generator state is the numpy stream's after as many draws as packets it tried to send."""
    import sgn
    kind, payload = END_CASES[case]
    V, n = len(END_LOSSES), hosts.n
    d, st = sim.digests(0, n), sim.stats()
    sent = d["n_sent"].astype(np.int64)
    on_all = hosts.node_id == END_LOSS_ALL
    empty = np.full(n, payload == 0) if kind == "periodic" else (np.arange(n) >= V) & (payload == 0)
    assert st["packets_sent"] > 1000 and st["packets_unknown_dst"] == 0, st
    assert (sent[on_all & ~empty] == 0).all(), sent[on_all]
    assert (sent[(END_LOSSES[hosts.node_id] <= 0.5) & (np.arange(n) >= V)] > 0).all(), sent
    assert (sent[empty] > 0).all(), sent
    if kind == "periodic":
        assert (st["packets_loss_dropped"] == 0) == (payload == 0), st
    else:
        assert st["packets_loss_dropped"] > 0, st
    # a host all of whose packets are empty loses none: it drew once per packet sent
    if empty.any():
        assert np.array_equal(d["rng"][empty], state_after(hosts.seed[empty], sent[empty]))
    if trace is not None:
        s = trace[trace["kind"] == sgn.TRACE_SEND]
        s = s[np.lexsort((s["seq"], s["host"]))]
        assert (s["flags"] <= 1).all()
        tried = np.bincount(s["host"], minlength=n)
        lost = np.bincount(s["host"][s["flags"] == 1], minlength=n)
        assert np.array_equal(tried - lost, sent)
        assert (lost[empty] == 0).all(), lost
        assert (tried[on_all] > 0).all(), tried[on_all]
        assert np.array_equal(s["rng_pos"], np.concatenate([np.arange(1, k + 1) for k in tried]))
        assert np.array_equal(d["rng"], state_after(hosts.seed, tried))


def probe_sends(trace, probes):
    """For probes on hosts 0..len-1: the SEND record of probe host v with rng_pos == index + 1
    (the draw counter after that packet's draw), or None."""
    import sgn
    t = trace[(trace["kind"] == sgn.TRACE_SEND) & (trace["host"] < len(probes))]
    want = np.array([p.index + 1 for p in probes], dtype=np.uint64)
    hit = t[t["rng_pos"] == want[t["host"]]]
    out = [None] * len(probes)
    for r in hit:
        assert out[r["host"]] is None, r
        out[r["host"]] = r
    return out


def probe_batch_positions(trace, probes):
    """Where each probe's packet sits in its send: (j, n) = its position among the n packets its
    host sent to the same peer at the same instant (one send_packet loop of the relay; the
    batched loss test takes packets 0 .. 8 * (n // 8) - 1 of a send eight draws at a time)."""
    import sgn
    out = []
    s = trace[(trace["kind"] == sgn.TRACE_SEND) & (trace["host"] < len(probes))]
    for v, p in enumerate(probes):
        h = s[s["host"] == v]
        h = h[np.argsort(h["rng_pos"])]
        k = int(np.nonzero(h["rng_pos"] == p.index + 1)[0][0])
        same = (h["a"] == h["a"][k]) & (h["peer"] == h["peer"][k])
        lo = hi = k
        while lo > 0 and same[lo - 1]:
            lo -= 1
        while hi + 1 < len(h) and same[hi + 1]:
            hi += 1
        out.append((k - lo, hi - lo + 1))
    return out


def check_probe_sends(trace, probes, who):
    """Every probe's packet is in the trace and was dropped or kept as the numpy stream says."""
    bad = []
    for v, (p, r) in enumerate(zip(probes, probe_sends(trace, probes))):
        if r is None:
            bad.append((who, "unreached", v, p.cls, p.index))
        elif int(r["flags"]) != (1 if p.drop else 0):
            bad.append((who, "wrong decision", v, p.cls, p.index, hex(p.x), hex(p.Th), int(r["flags"])))
    assert not bad, bad
