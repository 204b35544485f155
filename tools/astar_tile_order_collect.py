"""Turns what tools/astar_tile_order_measure.sh left in a directory into profiles/astar_tile_order_time.json and
profiles/astar_tile_order_pmc.json (parent commit's library against this tree's, taking turns on one GPU).

  python tools/astar_tile_order_collect.py <output directory of the measure script>"""
import csv
import glob
import json
import os
import re
import sys

src = sys.argv[1]
dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
SIDES = ("parent", "new")


def runs(map_, side):
    out = []
    for p in sorted(glob.glob(os.path.join(src, f"bench_{map_}_{side}_*.json"))):
        out.append(json.load(open(p))["value"])
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


time = {"command": "python bench.py [--map M] (plain run, defaults: 64 steps, 16 warm-up, 2 contexts, 32 steps per call), a fresh process per run, "
                   "the parent commit's library (SC_LIB_PATH) and this tree's taking turns on one MI355X in one session",
        "unit": "plans/s"}
for m in ("salt20", "salt05", "blocks"):
    p, n = runs(m, "parent"), runs(m, "new")
    time[m] = {"parent": p, "new": n, "parent_min_max": [min(p), max(p)], "new_min_max": [min(n), max(n)],
               "parent_median": median(p), "new_median": median(n), "median_ratio": median(n) / median(p)}
time["salt20"]["ranges_do_not_overlap"] = min(time["salt20"]["new"]) > max(time["salt20"]["parent"])
for m in ("salt05", "blocks"):
    time[m]["new_median_not_below_parent_lowest"] = time[m]["new_median"] >= min(time[m]["parent"])
full = {}
for side in SIDES:
    j = json.load(open(os.path.join(src, f"bench_full_{side}.json")))
    full[side] = {"value": j["value"], "value_min": j["value_min"], "value_max": j["value_max"], "value_depth1": j["value_depth1"],
                  "config3_one_gpu_share_plans_per_s": j["config3_one_gpu_share"]["plans_per_s"],
                  "config3_ms_astar": j["config3_one_gpu_share"]["ms_astar"],
                  "other_maps": {k: v["value"] for k, v in j["other_maps"].items()},
                  "kernels_ms_per_launch_on_context0": {k: v["ms_per_launch_on_context0"] for k, v in j["kernels"].items()},
                  "astar_expansions_per_step": j["astar"]["expansions_per_step_rank0"]}
time["bench_full_once_each"] = full
json.dump(time, open(os.path.join(dst, "astar_tile_order_time.json"), "w"), indent=1)


def top3(path, counter):
    """mean over the three largest dispatches of astar_kernel*: the three 6144-query launches"""
    acc = {}
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] == counter and "astar_kernel" in r["Kernel_Name"]:
            acc[r["Dispatch_Id"]] = acc.get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
    v = sorted(acc.values(), reverse=True)[:3]
    return sum(v) / len(v)


pmc = {"workload": "tools/astar_saturation.py salt20 6144 under rocprofv3 --kernel-trace --pmc <group> (one pass per group: TCC_HIT_sum TCC_MISS_sum; "
                   "TCC_ATOMIC_sum; FETCH_SIZE; WRITE_SIZE), mean of the three 6144-query launches; 6144 copies of ONE query: its time is "
                   "informative only"}
for side in SIDES:
    c = {}
    for grp in ("TCC_HIT_sum_TCC_MISS_sum", "TCC_ATOMIC_sum", "FETCH_SIZE", "WRITE_SIZE"):
        path = glob.glob(os.path.join(src, f"pmc_{side}_{grp}", "**", "a_counter_collection.csv"), recursive=True)[0]
        for name in grp.replace("_sum_", "_sum ").split():
            c[name] = top3(path, name)
    log = open(os.path.join(src, f"pmc_{side}_FETCH_SIZE.log")).read()
    m = re.search(r"x6144: ([\d.]+) ms, (\d+) expansions / (\d+) popped / (\d+) steps each -> ([\d.]+) G", log)
    ms, ex, pop, steps = float(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))
    nexp = 6144 * ex
    pmc[side] = {"counters_per_launch": c, "expansions_per_query": ex, "popped_per_query": pop, "steps_per_query": steps,
                 "TCC_HIT_per_expansion": c["TCC_HIT_sum"] / nexp, "TCC_MISS_per_expansion": c["TCC_MISS_sum"] / nexp,
                 "L2_requests_per_expansion": (c["TCC_HIT_sum"] + c["TCC_MISS_sum"]) / nexp,
                 "L2_miss_fraction": c["TCC_MISS_sum"] / (c["TCC_HIT_sum"] + c["TCC_MISS_sum"]),
                 "L2_atomic_requests_per_expansion": c["TCC_ATOMIC_sum"] / nexp,
                 "HBM_bytes_read_per_expansion": c["FETCH_SIZE"] * 1024 / nexp, "HBM_bytes_written_per_expansion": c["WRITE_SIZE"] * 1024 / nexp,
                 "launch_ms_under_profiler": ms}
json.dump(pmc, open(os.path.join(dst, "astar_tile_order_pmc.json"), "w"), indent=1)
print(json.dumps({"time": {k: v for k, v in time.items() if k in ("salt20", "salt05", "blocks")},
                  "pmc": {s: {k: v for k, v in pmc[s].items() if k != "counters_per_launch"} for s in SIDES}}, indent=1))
