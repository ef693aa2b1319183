"""Event runs gathered per round over bench.py's timed steps on config C (the loop of
`bench.py --gpus 1 --steps 20 --warmup 5`), with the packets sent and popped per round and the
round kernel's average launch time; one JSON line. SGN_LIB selects the build."""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
import sgn  # noqa: E402

steps, warm, rps = 20, 5, 100
g, used, hosts, cfg, tr = bench.build_workload(100_000, 1000)
ctx = sgn.Context(device=0, flags=2)
ctx.routes_build(g, used)
ctx.hosts_set(hosts)
ctx.sim_init(cfg, tr)
for _ in range(warm):
    ctx.run(rps)
s0 = ctx.stats()
k0 = ctx.kernel_times()["k_rounds"]
for _ in range(steps):
    ctx.run(rps)
s1 = ctx.stats()
k1 = ctx.kernel_times()["k_rounds"]
d = {k: s1[k] - s0[k] for k in s1}
r = d["rounds"]
info = ctx.engine_info()
print(json.dumps({"lib": str(sgn.LIB_PATH.name), "rounds": r, "event_runs_per_round": d["event_runs"] / r,
                  "popped_per_round": d["packet_events_popped"] / r,
                  "sent_per_round": d["packets_sent"] / r,
                  "avg_launch_us": (k1[1] - k0[1]) / (k1[0] - k0[0]) * 1e3,
                  "engine": {k: info[k] for k in ("slab_extensions", "big_slab_pieces", "calendar_spill_runs")}}))
ctx.close()
