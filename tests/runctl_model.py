"""The CPU side of the run-control sweep (tests/test_gpu_runctl_fuzz.py): seeded programs of
pauses, saves, rewinds, file round trips and takes over the scenarios of test_gpu_fuzz.draw, and
what every step of such a program must give, worked out from the oracle's ONE uninterrupted run.
Pure Python and numpy: nothing here touches a GPU (tests/test_runctl_model.py checks it there).

A program is a list of operations:
  ("run", k)               k rounds (None: to the end)
  ("run_until", u, back)   a time target, made concrete by resolve(): t = S0 + a fraction of the stop
                           time that lies u of the way from the current window start to the stop time
                           (back: u of the way from S0 to the current window start, so t <= that
                           start and the call runs nothing). Never a multiple of 1 ms.
  ("save", slot)           slot "a", "b" or "c"
  ("restore", slot)
  ("export_import", slot)  the slot's snapshot to a file and back; the imported one takes the slot
  ("fresh", slot)          the slot's snapshot to a file, into a NEW context of the same simulation,
                           which carries on; the old context goes, and its other snapshots with it
  ("take",)                sgn_trace_take of everything pending
  ("take_small", which)    arrays one record ("records") or one span ("spans") too small: SGN_ERANGE
                           with both needed counts, nothing taken
Every program starts with a pause inside the run and a save, and ends with a pause further on and a
rewind to that save — the save / rewind pair the sweep is about — then run() to the end and, traced,
a last take; what lies between is drawn. Four programs in ten also save at the closing pause and,
after the rewind, restore that save: a snapshot AHEAD of the position.

The trace cursor (DESIGN.md §7b "The cursor", "Snapshots") is TraceLedger, in records produced:
n records produced so far, base of them handed out, held the end of what the buffer holds in place.
  run to round r      n = P(r); held = max(held, n)
  take                returns [base, n); base = held = n (a take of nothing changes nothing)
  restore, own save   n = N; base = min(base, N) — the buffer must still hold [base, N): held >= N
                      when base < N, else the restore is refused (SGN_ESTATE, nothing changes);
                      held = N when the cursor moved back
  export, own save    the file holds [b, N), b = min(base, N), under the same condition
  restore, imported   n = held = N; base = the file's b
P(r) is the length of the oracle's trace (filtered to the traced hosts) after r rounds; the oracle
appends in production order, so a take is a slice of that trace, sorted by (host, seq).
"""
import numpy as np

from test_gpu_fuzz import draw
from test_gpu_snapshot import S0, assert_state, state  # noqa: F401 (the comparers, for the sweep's tests)
from test_gpu_trace_capture import check_take, only, same_records, srt  # noqa: F401

SLOTS = "abc"
MS = 1_000_000
KINDS = ("run", "run_until", "save", "restore", "export_import", "fresh", "take", "take_small")
#         run   until  save  restore  exp_imp  fresh  take  take_small
_W_PLAIN = (0.18, 0.14, 0.16, 0.18, 0.18, 0.16, 0.0, 0.0)
_W_TRACED = (0.15, 0.13, 0.17, 0.17, 0.12, 0.0, 0.13, 0.13)


def draw_case(i, trace=None):
    """Case i: test_gpu_fuzz.draw(i)'s scenario, environment and trace flag (trace: overrides the
    flag), a host set for half of the traced cases, and a program from its own generator."""
    kw, env, tr = draw(i)
    if trace is not None:
        tr = trace
    r = np.random.default_rng(5000 + i)
    n_ops = int(r.integers(6, 13))
    hosts = None
    if tr and r.random() < 0.5:
        k = int(r.integers(1, 9))  # 1-8 hosts, host 0 and host n-1 always among them (so: at least two)
        others = r.choice(np.arange(1, kw["n"] - 1), size=max(0, k - 2), replace=False)
        hosts = sorted({0, kw["n"] - 1} | {int(h) for h in others})
    first = SLOTS[int(r.integers(0, 3))]
    ops = [("run_until", float(r.uniform(0.05, 0.3)), False), ("save", first)]
    filled, keep = {first}, first
    w = np.array(_W_TRACED if tr else _W_PLAIN)
    ahead = bool(r.random() < 0.4)  # a save at the far pause too, and after the closing rewind forward to it
    while len(ops) < n_ops - 2 - 2 * ahead:
        kind = KINDS[int(r.choice(len(KINDS), p=w / w.sum()))]
        if kind == "run":
            ops.append(("run", int(r.integers(1, 81))))
        elif kind == "run_until":
            ops.append(("run_until", float(r.uniform(0.02, 0.98)), bool(r.random() < 0.125)))
        elif kind == "save":  # (the first save keeps its slot for the closing rewind)
            ops.append(("save", [s for s in SLOTS if s != keep][int(r.integers(0, 2))]))
            filled.add(ops[-1][1])
        elif kind == "take":
            ops.append(("take",))
        elif kind == "take_small":
            ops.append(("take_small", "records" if r.random() < 0.5 else "spans"))
        else:
            slot = sorted(filled)[int(r.integers(0, len(filled)))]
            if kind == "fresh":
                slot = keep
                filled = {keep}
            ops.append((kind, slot))
    ops.append(("run_until", float(r.uniform(0.4, 0.8)), False))
    far = [s for s in SLOTS if s != keep][int(r.integers(0, 2))]
    ops += [("save", far), ("restore", keep), ("restore", far)] if ahead else [("restore", keep)]
    ops.append(("run", None))
    if tr:
        ops.append(("take",))
    return {"kw": kw, "env": env, "trace": tr, "hosts": hosts, "program": ops}


def oracle_rounds(oracle, args, trace, every_state=True):
    """The oracle stepped a round at a time to the end, once: the window start, the trace length and
    state() after every round (index 0: before the first)."""
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=trace)
    n = hosts.n
    count = (lambda: int(o.L.ora_sim_trace_count(o.h))) if trace else (lambda: 0)
    windows, lens, states = [o.window()[0]], [count()], [state(o, n)]
    while o.window()[2]:
        o.round()
        windows.append(o.window()[0])
        lens.append(count())
        states.append(state(o, n) if every_state else None)
    if not every_state:
        states[-1] = state(o, n)
    return {"o": o, "n": n, "windows": windows, "lens": lens, "states": states,
            "stop": int(cfg.stop_time_ns), "trace": o.trace() if trace else None}


class TraceLedger:
    """The trace cursor over the oracle's trace `trace` (production order), `lens[r]` its length
    after r rounds, restricted to `hosts` (None: all)."""

    def __init__(self, trace, lens, hosts=None):
        mask = np.ones(len(trace), bool) if hosts is None else np.isin(trace["host"], np.asarray(hosts, np.uint32))
        csum = np.concatenate([[0], np.cumsum(mask)])
        self.P = [int(csum[k]) for k in lens]
        self.recs = trace[mask]
        self.n = self.base = self.held = 0
        self.slots = {}  # slot -> (N, None) saved here, (N, b) imported

    def produced(self, r):
        return self.recs[: self.P[r]]

    def pending(self):
        return self.n - self.base

    def run_to(self, r):
        self.n = self.P[r]
        self.held = max(self.held, self.n)

    def take(self):
        out = srt(self.recs[self.base:self.n])
        if len(out):  # (a take of nothing leaves the cursor where it is)
            self.base = self.held = self.n
        return out

    def peek(self):
        return srt(self.recs[self.base:self.n])

    def save(self, slot):
        self.slots[slot] = (self.n, None)

    def holds(self, slot):
        """Whether the buffer still holds the records a restore or an export of the slot needs."""
        N, b = self.slots[slot]
        return b is not None or self.base >= N or self.held >= N

    def export_import(self, slot):
        N, b = self.slots[slot]
        if not self.holds(slot):
            return False
        self.slots[slot] = (N, min(self.base, N) if b is None else b)
        return True

    def restore(self, slot):
        N, b = self.slots[slot]
        if not self.holds(slot):
            return False
        if b is not None:
            self.base, self.held = b, N
        elif self.base > N:  # (the cursor moves back: what lay past it goes)
            self.base = self.held = N
        self.n = N
        return True


def resolve(program, windows, stop_ns, ledger=None):
    """The program against the oracle's window starts (windows[r]: after r rounds; the last is the
    end): per operation {op, round (after it), ret (the rounds the call must report, for the
    running calls), t (run_until's target), refused, pending, take (expected records), needed}.
    ledger: a TraceLedger, advanced with the program (traced cases)."""
    R = len(windows) - 1
    cur, slots, steps = 0, {}, []
    for op in program:
        st = {"op": op, "ret": None, "t": None, "refused": False, "take": None, "needed": None}
        kind = op[0]
        if kind == "run":
            to = R if op[1] is None else min(R, cur + op[1])
            st["ret"], cur = to - cur, to
        elif kind == "run_until":
            ws = windows[cur] - S0
            rel = int(op[1] * ws) if op[2] else ws + int(op[1] * (stop_ns - ws))
            if rel % MS == 0 and not (op[2] and rel == 0):
                rel += 12_345 if not op[2] else -1
            t = S0 + rel
            to = cur
            if cur < R and t > windows[cur]:
                to = next((r for r in range(cur + 1, R) if windows[r] >= t), R)
            st["t"], st["ret"], cur = t, to - cur, to
        elif kind == "save":
            slots[op[1]] = cur
            if ledger:
                ledger.save(op[1])
        elif kind == "restore":
            if ledger and not ledger.restore(op[1]):
                st["refused"] = True
            else:
                cur = slots[op[1]]
        elif kind == "export_import":
            if ledger and not ledger.export_import(op[1]):
                st["refused"] = True
        elif kind == "fresh":
            assert ledger is None, "fresh is not drawn for traced cases"
            cur = slots[op[1]]
            slots = {op[1]: cur}
        elif kind == "take":
            st["take"] = ledger.take()
        elif kind == "take_small":
            want = ledger.peek()
            st["needed"] = (len(want), len(np.unique(want["host"])))
            # (one span of one is no array at all, and a null span array asks for no spans: records then)
            st["small"] = op[1] if st["needed"][1] > 1 else "records"
        if ledger:
            if kind in ("run", "run_until"):
                ledger.run_to(cur)
            st["pending"] = ledger.pending()
        st["round"] = cur
        steps.append(st)
    return steps


def cached_edges(trace, windows, server=0):
    """The round edges at which the server holds a cached packet: an IF_POP of the server at or
    before the window start whose SEND (the k-th SEND is the k-th IF_POP's) is later than it.
    trace: the oracle's, sorted by (host, seq). Returns [(round, payload of the cached packet)]."""
    from test_gpu_train_merge import server_sends
    tp, ts, _, pay, _ = server_sends(trace, server)
    out = []
    for r in range(1, len(windows) - 1):
        k = np.nonzero((tp <= windows[r]) & (ts > windows[r]))[0]
        if len(k):
            out.append((r, int(pay[k[0]])))
    return out


def cached_round(name, trace, windows):
    """The save round of the train-merge cases: the first edge with a cached packet that leaves
    five rounds to run; for cached_last_then_other_train the first whose cached packet is a
    train's short last one."""
    from test_gpu_train_merge import CASES, MSS
    edges = [(r, p) for r, p in cached_edges(trace, windows) if r + 5 < len(windows) - 1]
    if name == "cached_last_then_other_train":
        last = CASES[name]["file_bytes"] % MSS
        short = [e for e in edges if e[1] == last]
        edges = short or edges
    assert edges, name
    return edges[0][0]
