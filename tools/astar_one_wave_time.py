"""The one-wavefront A* kernel (SC_ASTAR_DUAL=0: what the overflow retry pass and sc_astar_gfield run) timed alone: one
1024^2 salt20 grid, the benchmark's 1024 queries, the context's own timing of K_ASTAR (prep + search + retry launch),
2 warm-ups then 7 repeats per process.
usage: astar_one_wave_time.py --out FILE [--rounds R] NAME=LIB [NAME=LIB ...]
Every library is timed in a fresh process of its own (SC_LIB_PATH), the libraries alternating, R rounds; FILE gets the raw
repeats, the median and the spread (max - min) per library and, with a library named `parent`, whether every other
library's median is within the parent's median + the parent's spread."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sea-current_amd", "python")); sys.path.insert(0, ROOT)
import numpy as np


def child():
    import torch
    import sea_current_amd as sc
    from sea_current_amd import synth
    ctx = sc.Context(0)
    d2 = ctx.edt(torch.from_numpy(synth.salt_grid(1024, 1024, 0.20)).cuda())
    ctx.synchronize()
    s, g = synth.queries(d2.cpu().numpy() >= 1, 1024)
    s, g = torch.from_numpy(s).cuda(), torch.from_numpy(g).cuda()
    ctx.set_timing(True)
    ms = []
    for _ in range(2 + 7):
        ctx.reset_timing()
        out = ctx.astar_batch(d2, s, g, Lmax=4096)
        ctx.synchronize()
        ms.append(ctx.get_timing(sc.K_ASTAR)[0])
    assert int((out["status"] != 0).sum()) == 0
    print(json.dumps({"ms": ms[2:], "expansions": int(ctx.astar_debug_stats(1024)[0].sum())}), flush=True)
    ctx.close()


def main():
    a = sys.argv[1:]
    out = a[a.index("--out") + 1]
    rounds = int(a[a.index("--rounds") + 1]) if "--rounds" in a else 3
    libs = [x.split("=", 1) for x in a if "=" in x]
    res = {n: {"lib": os.path.relpath(p, ROOT), "all_ms": [], "expansions": None} for n, p in libs}
    for r in range(rounds):
        for n, p in libs:
            env = dict(os.environ, SC_ASTAR_DUAL="0", SC_LIB_PATH=os.path.abspath(p))
            # a child that faults, aborts or runs into its limit ends the whole measurement: nothing more is started
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, timeout=240, check=True)
            j = json.loads(o.stdout.decode().strip().splitlines()[-1])
            res[n]["all_ms"] += j["ms"]
            assert res[n]["expansions"] in (None, j["expansions"])
            res[n]["expansions"] = j["expansions"]
            print(r, n, ["%.3f" % v for v in j["ms"]], flush=True)
    for v in res.values():
        v["median_ms"] = float(np.median(v["all_ms"]))
        v["spread_ms"] = float(max(v["all_ms"]) - min(v["all_ms"]))
    doc = {"workload": "sc_astar_batch, 1024^2 salt20, 1024 queries (synth.queries), SC_ASTAR_DUAL=0, K_ASTAR per call; per process 2 warm-ups "
                       "then 7 repeats, %d processes per library, the libraries alternating" % rounds, "libraries": res}
    if "parent" in res:
        doc["bound"] = "median <= parent median + parent spread (max - min)"
        doc["within_bound"] = {n: v["median_ms"] <= res["parent"]["median_ms"] + res["parent"]["spread_ms"] for n, v in res.items() if n != "parent"}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in doc if k != "libraries"}), {n: (v["median_ms"], v["spread_ms"]) for n, v in res.items()})


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
