"""A numpy / Python model of the router delay report (sgn_delay_*), for the CPU tests (on the
oracle's trace) and as the expected value of the GPU tests.

The kernels pair the k-th exit of a host with its k-th POP (rank). The model pairs by KEY instead:
an exit (DELIVER or CODEL_DROP) belongs to the pending POP of the same (host, peer, c) = (host,
source host, source event id). It shares nothing with the kernels' method; pairs_by_rank() is here
only so that the CPU tests can show on the oracle's trace that the two matches agree."""
import numpy as np

import sgn

POP, DELIVER, CODEL_DROP = sgn.TRACE_POP, sgn.TRACE_DELIVER, sgn.TRACE_CODEL_DROP
INVALID = sgn.EMUTIME_INVALID
BINS = sgn.DELAY_BINS


def delay_bin(d):
    """Bin 0: 0; bin k (1..46): 2^(k-1) <= d < 2^k; bin 47: from 2^46 up."""
    return min(int(d).bit_length(), BINS - 1)


def ordered(recs):
    """recs by (host, seq)."""
    return recs[np.lexsort((recs["seq"], recs["host"]))]


def pairs_by_key(recs):
    """(pop index, exit index) of every exit whose POP is in recs, matched on (host, peer, c); recs
    ordered by (host, seq). Exits without a POP in recs are left out."""
    pending, out = {}, []
    for i, (k, h, p, c) in enumerate(zip(recs["kind"].tolist(), recs["host"].tolist(), recs["peer"].tolist(), recs["c"].tolist())):
        if k == POP:
            assert (h, p, c) not in pending, (h, p, c)
            pending[(h, p, c)] = i
        elif k in (DELIVER, CODEL_DROP) and (h, p, c) in pending:
            out.append((pending.pop((h, p, c)), i))
    return out


def pairs_by_rank(recs):
    """(pop index, exit index): the k-th exit of a host with its k-th POP; recs ordered by (host, seq)."""
    out = []
    kind, host = recs["kind"], recs["host"]
    for h in np.unique(host):
        at = np.nonzero(host == h)[0]
        pops = at[kind[at] == POP]
        exits = at[(kind[at] == DELIVER) | (kind[at] == CODEL_DROP)]
        assert len(exits) <= len(pops), (h, len(exits), len(pops))
        out += list(zip(pops[: len(exits)].tolist(), exits.tolist()))
    return out


class DelayModel:
    """The report's state: per host the unknown entries left, the pending POPs by key (insertion
    order = pop order), the accumulators; both histograms."""

    def __init__(self, standing0=None, host_lo=0):
        self.unknown = {}
        if standing0 is not None:
            self.unknown = {host_lo + i: int(v) for i, v in enumerate(standing0) if v}
        self.pending = {}  # host -> {(peer, c): pop time}
        self.acc = {}      # host -> [delivered, dropped, sum_delivered, sum_dropped, max, unmatched]
        self.hist = np.zeros((2, BINS), np.uint64)
        self.folds = self.records = 0

    def fold(self, piece):
        """One interval's records, in any order."""
        piece = ordered(piece)
        self.folds += 1
        self.records += len(piece)
        for k, h, p, c, a in zip(piece["kind"].tolist(), piece["host"].tolist(), piece["peer"].tolist(), piece["c"].tolist(),
                                 piece["a"].tolist()):
            if k == POP:
                q = self.pending.setdefault(h, {})
                assert (p, c) not in q
                q[(p, c)] = a
            elif k in (DELIVER, CODEL_DROP):
                acc = self.acc.setdefault(h, [0, 0, 0, 0, 0, 0])
                q = self.pending.get(h, {})
                if (p, c) not in q:  # a packet that stood at the router before the report began
                    assert self.unknown.get(h, 0) > 0, ("an exit without a POP", h, p, c)
                    self.unknown[h] -= 1
                    acc[5] += 1
                    continue
                assert self.unknown.get(h, 0) == 0, ("a known packet leaves before an unknown one", h)
                d = a - q.pop((p, c))
                assert d >= 0
                x = 1 if k == CODEL_DROP else 0
                acc[x] += 1
                acc[2 + x] += d
                acc[4] = max(acc[4], d)
                self.hist[x, delay_bin(d)] += 1

    def clear(self):
        self.acc = {}
        self.hist[:] = 0
        self.folds = self.records = 0

    def result(self):
        """(rows, info): rows as DELAY_ROW_DTYPE ascending by host, info with the keys of Delay.info
        that do not describe a round edge."""
        hosts = sorted(set(self.acc) | {h for h, q in self.pending.items() if q} | {h for h, v in self.unknown.items() if v})
        rows = np.zeros(len(hosts), sgn.DELAY_ROW_DTYPE)
        keep = []
        best = None
        for i, h in enumerate(hosts):
            acc = self.acc.get(h, [0] * 6)
            q = self.pending.get(h, {})
            unk = self.unknown.get(h, 0)
            r = rows[i]
            r["host"], r["standing"], r["unmatched"] = h, unk + len(q), acc[5]
            r["delivered"], r["dropped"], r["delay_sum_delivered"], r["delay_sum_dropped"], r["delay_max"] = acc[:5]
            r["standing_oldest"] = INVALID if unk or not q else next(iter(q.values()))
            keep.append(bool(r["standing"] or r["unmatched"] or r["delivered"] or r["dropped"]))
            if acc[0] + acc[1] and (best is None or acc[4] > best[0]):
                best = (acc[4], h)
        rows = rows[np.array(keep, bool)] if len(hosts) else rows
        info = {
            "folds": self.folds, "records": self.records, "rows": len(rows),
            "total": [int(rows[f].sum(dtype=np.uint64)) for f in sgn.DELAY_TOTALS],
            "delay_max": best[0] if best else 0, "delay_max_host": best[1] if best else 0,
            "hist_delivered": self.hist[0].tolist(), "hist_dropped": self.hist[1].tolist(),
        }
        return rows, info


def run_model(recs, piece_ends=None, standing0=None, host_lo=0):
    """The model on recs cut at piece_ends (default: one piece): (rows, info)."""
    m = DelayModel(standing0, host_lo)
    ends = [len(recs)] if piece_ends is None else [int(e) for e in piece_ends]
    a = 0
    for e in ends:
        m.fold(recs[a:e])
        a = e
    return m.result()


def assert_report(delay, rows, info, what=""):
    """A sgn.Delay against the model's (rows, info): every row field and every info key the model has."""
    for k, v in info.items():
        assert delay.info[k] == v, (what, k, delay.info[k], v)
    assert len(delay.rows) == len(rows), (what, len(delay.rows), len(rows))
    for f in sgn.DELAY_ROW_DTYPE.names:
        bad = np.nonzero(delay.rows[f] != rows[f])[0]
        assert len(bad) == 0, (what, f, delay.rows[bad[:3]], rows[bad[:3]])
