#!/usr/bin/env python3
"""bench.py -- plans/sec of the planning hot path on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path over one batch: EDT of the 1024x1024 occupancy grid (recomputed
every step: the grid is an input) + batched A* over this rank's start-goal queries [+ all-gather of
the result paths over RCCL when N > 1].  Inputs (grid, queries) are resident in HBM before the timed region.

  python bench.py --gpus N --steps K --warmup W
  N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line.  Weak scaling: every rank plans `--queries` (default 1024) queries;
value = (N * queries * K) / max-over-ranks time of the K steps.  Query i is the same on any rank count.

Consecutive steps are independent batches: step k has its OWN grid (seed SEED_GRID + k) and its own query block
(queries k * Qtot .. of the generator, drawn on that grid).  No entry point of the library blocks the host, so the K
steps are simply enqueued, `--group` consecutive steps per library call, calls round-robin on `--depth` contexts (a
context = one HIP stream + its scratch); one host thread, one synchronisation at the end.  The K-step region is timed
`--repeats` times (barrier + synchronise on both sides of each, max over ranks): `value` is the MEDIAN repeat, minimum
and maximum beside it.  A plain run times the region once (exactly K timed steps); `--full` times it 5 times by default.

A plain run does only what the headline needs: set up, warm up, time the K steps, write the outputs (`--dump-outputs
DIR`: the last timed step's distance map and A* results [and gathered paths], as float64 .npy, at most 64 MB) and print
the line.  Everything below runs only with `--full`.

  value_depth1 -- one call per step on one stream (what ONE call of 1024 queries gets); per-kernel times of the steps.

Also measured with --full (outside the timed steps, reported in the same line):
  roofline     -- the EDT kernels on a batch of 64 grids (one 1024^2 grid is 5.2 MB: launch-bound
                  and cache-resident), timed with HIP events on the stream the kernels run on;
                  achieved = 5 B/cell * cells / (colbits + band time).  Other map families and 4096^2 beside it.
  configs2     -- BASELINE configs[2]: the same step plus TOPP-RA (6 joints, 200 stages) of 1024 plans.
  replan_stream-- BASELINE configs[4] on one GPU.
  cpu_baseline -- the CPU oracle (our C restatement; the reference has no grid path and cannot be
                  built here) on a bounded sample of the same queries, all host cores.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "sea-current_amd", "python")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
EDT_BYTES_PER_CELL = 5  # read occ 1 B + write d2 4 B

FAMILIES = ("salt05", "salt20", "blocks")


def make_grid(name, W, H, seed=None):
    from sea_current_amd import synth
    kw = {} if seed is None else {"seed": seed}
    if name == "salt05":
        return synth.salt_grid(W, H, 0.05, **kw)
    if name == "salt20":
        return synth.salt_grid(W, H, 0.20, **kw)
    if name == "blocks":
        return synth.block_grid(W, H, 0.20, **kw)
    if name == "open":     # open space: 2e-5 of the cells occupied, distances of hundreds of cells (EDT legs only)
        return synth.salt_grid(W, H, 2e-5, **kw)
    raise ValueError(name)


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(dirname, d2, out, gath, lmax, gathered_rows, Qloc):
    """--dump-outputs: what one timed step handed its caller, as float64 .npy under `dirname` (every int32 value exact).
    d2 [H, W] distance map; path [Q, lmax] with the cells past each query's `len` set to -1 (never written by the kernel);
    len / cost / status [Q]; with the gather on, the gathered len / cost / status of this step for every rank and the cells
    of their paths.  Arrays larger than their share of 64 MB keep a fixed seeded sample of their rows, and `<name>_rows`
    holds the row numbers kept."""
    ln = out["len"].cpu().numpy()
    pth = out["path"].cpu().numpy()
    pth = np.where(np.arange(lmax)[None, :] < np.clip(ln, 0, lmax)[:, None], pth, -1)
    arrays = {"d2": d2.cpu().numpy(), "path": pth, "len": ln, "cost": out["cost"].cpu().numpy(), "status": out["status"].cpu().numpy()}
    if gath is not None:
        off = gath["offsets"].cpu().numpy()
        rows = np.concatenate([np.arange(r0, r0 + Qloc) for r0 in gathered_rows])
        for k in ("len", "cost", "status"):
            arrays["gather_" + k] = gath[k].cpu().numpy()[rows]
        cells = gath["cells"].cpu().numpy()
        arrays["gather_cells"] = np.concatenate([cells[off[r0]:off[r0 + Qloc]] for r0 in gathered_rows])
        arrays["gather_truncated"] = gath["truncated"].cpu().numpy()
    total = sum(8 * a.size for a in arrays.values())
    scale = min(1.0, 0.9 * DUMP_BYTES_MAX / total)       # 10 % left for the row numbers of sampled arrays
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        a = a.astype(np.float64)
        if scale < 1.0 and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * scale))
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
            a = a[rows]
            np.save(os.path.join(dirname, name + "_rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1024, help="queries per GPU per step")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--map", default="salt20", choices=list(FAMILIES),
                    help="obstacle family of the headline numbers (the other two are reported under other_maps)")
    ap.add_argument("--only-main-map", action="store_true")
    ap.add_argument("--depth", type=int, default=2,
                    help="contexts (streams) the steps are enqueued on round-robin; 1 = strictly sequential steps")
    ap.add_argument("--group", type=int, default=0,
                    help="consecutive steps handed to the library as ONE call (EDT with batch = group, sc_astar_batch_multi over "
                         "group x queries): the launch then has one tail for `group` steps; 1 = one call per step; "
                         "0 = the largest divisor of --steps that is <= 32 (20 steps: one call of 20; 64 steps: 32 per call, "
                         "alternating between the contexts), so that exactly --steps steps are timed.  Measured: 20 steps as "
                         "2 x 10 on two contexts 478 k plans/s, as one call 559 k; 64 steps as 4 x 16, 2 x 32 or 1 x 64: 544-557 k")
    ap.add_argument("--repeats", type=int, default=None,
                    help="how many times the K-step region is timed (value = median); default 1, 5 with --full")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline: depth-1 run, per-kernel times, other maps, configs2, roofline, "
                         "TOPP-RA, replan stream, configs[3], smoothing, FMT*, CPU baseline and the gather checks")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float64, at most 64 MB in all)")
    ap.add_argument("--lmax", type=int, default=4096)
    ap.add_argument("--edt-batch", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--replan-frames", type=int, default=20,
                    help="frames of the dynamic-obstacle replan stream (BASELINE configs[4]) timed at N=1; 0 = skip")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world and world == 1 and args.gpus > 1:
        sys.exit("launch with torch.distributed.run for --gpus > 1")
    ngpu = torch.cuda.device_count()
    local_rank = local_rank % max(ngpu, 1)            # rehearsals with several ranks on one GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # The data path's only collective is the library's own (sc_allgather_paths, RCCL through the C ABI); the process
    # group is control plane only (barriers, the max over ranks of the step time, handing out the RCCL unique ids), on
    # gloo.  SC_BENCH_FORCE_DIST=1 drives the gather with a world of one (the only way to run it on a one-GPU box).
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    use_gather = world > 1 or bool(os.environ.get("SC_BENCH_FORCE_DIST"))

    import sea_current_amd as sc
    from sea_current_amd import synth, shard

    W = H = args.size
    Qloc = args.queries
    Qtot = Qloc * world
    q0, q1 = shard.rank_range(Qtot, world, rank)
    depth_max = max(1, args.depth)
    ctxs = [sc.Context(local_rank, use_torch_stream=False) for _ in range(depth_max)]
    ctx = ctxs[0]
    if use_gather:
        sys.stdout.flush()
        saved_stdout = os.dup(1)
        os.dup2(2, 1)    # RCCL prints its version banner on stdout when a communicator is created: keep stdout for the JSON line
        for c in ctxs:   # one communicator per context, created in the same order on every rank
            if world > 1:
                box = [sc.Context.comm_unique_id() if rank == 0 else None]
                dist.broadcast_object_list(box, src=0)
                uid = box[0]
            else:
                uid = sc.Context.comm_unique_id()
            c.comm_init(uid, world, rank)
        os.dup2(saved_stdout, 1)
        os.close(saved_stdout)

    def fence():
        for c in ctxs:
            c.synchronize()
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def alloc_out(G=1):
        return dict(path=torch.empty((G * Qloc, args.lmax), dtype=torch.int32, device=dev),
                    len=torch.empty(G * Qloc, dtype=torch.int32, device=dev),
                    cost=torch.empty(G * Qloc, dtype=torch.int32, device=dev),
                    status=torch.empty(G * Qloc, dtype=torch.int32, device=dev))

    # a rank's message carries at most this many path cells: 1/4 of the fixed-stride volume (mean path 519 of 4096 cells
    # on the headline map); a rank whose paths do not fit is flagged in `gather.truncated`
    cap_cells = Qloc * args.lmax // 4

    def run_map(family, steps, warmup, depth, with_toppra=False, group=1, repeats=1, timing=True):
        """Timed region for one obstacle family: `steps` x (EDT + batched A* [+ gather] [+ TOPP-RA]) on `depth` contexts,
        `group` consecutive steps per library call (every step still has its own grid buffer, distance map and results).
        timing=False: no per-kernel event brackets on context 0 and no statistics beyond the step time."""
        G = max(1, min(group, steps))
        # step k of a call: its own grid and its own queries (query block k of the generator, drawn from that grid's largest
        # free component -- needs each grid's traversable mask once, on the host)
        occ_hs = [make_grid(family, W, H, seed=synth.SEED_GRID + k) for k in range(G)]
        occ = torch.from_numpy(np.stack(occ_hs)).to(dev)
        d2s = [torch.empty((G, H, W), dtype=torch.int32, device=dev) for _ in range(depth)]
        ctx.edt(occ, out=d2s[0])
        ctx.synchronize()
        sg = [synth.queries(d2s[0][k].cpu().numpy() >= 1, q1 - q0, first=k * Qtot + q0) for k in range(G)]
        occ_h, s_h, g_h = occ_hs[0], sg[0][0], sg[0][1]
        start = torch.from_numpy(np.concatenate([a for a, _ in sg])).to(dev)
        goal = torch.from_numpy(np.concatenate([b for _, b in sg])).to(dev)
        qgrid = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int32), Qloc)).to(dev)
        outs = [alloc_out(G) for _ in range(depth)]
        gath = [None] * depth
        tp_args = None
        if with_toppra:
            pl = synth.toppra_plans(G * Qloc, dof=6, first=G * q0)   # a call's G steps hand their plans over together, like their queries
            tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            tp_args = (tt(pl["p0"]), tt(pl["p1"]), tt(pl["v0"]), tt(pl["v1"]), tt(-pl["vlim"]), tt(pl["vlim"]), tt(-pl["alim"]), tt(pl["alim"]))
        torch.cuda.synchronize()
        tp_last = [None]
        keep = []   # TOPP-RA outputs stay alive until the streams are idle (they are allocated by torch, used on our streams)

        def view(o, k):   # step k of a group's results
            return {kk: vv[k * Qloc:(k + 1) * Qloc] for kk, vv in o.items()}

        def run_steps(nsteps):
            assert nsteps % G == 0
            for i in range(nsteps // G):
                j = i % depth
                c = ctxs[j]
                c.edt(occ, out=d2s[j])
                if G == 1:
                    c.astar_batch(d2s[j][0], start, goal, r2=0, Lmax=args.lmax, out=outs[j])
                else:
                    c.astar_batch_multi(d2s[j], qgrid, start, goal, r2=0, Lmax=args.lmax, out=outs[j])
                if use_gather:
                    # one exchange per library call: this rank's G x Qloc results (step-major) to every rank; in the gathered
                    # arrays rank r's block is [r G Qloc, (r + 1) G Qloc), i.e. step k of rank r starts at (r G + k) Qloc
                    gath[j] = c.allgather_paths(outs[j], G * Qtot, G * cap_cells, bufs=gath[j])
                if with_toppra:
                    tp = c.toppra(*tp_args, N=200)
                    tp_last[0] = (tp, c.toppra_sample(tp_args[0], tp_args[1], tp_args[2], tp_args[3], tp["x"], tp["t"], 0.02, 512))
                    keep.append(tp_last[0])

        steps = ((steps + G - 1) // G) * G              # whole groups (the default group divides --steps; an explicit --group may round K up: reported)
        run_steps(((max(warmup, depth * G) + G - 1) // G) * G)   # every context allocates its scratch on its first call: not timed
        fence()
        keep.clear()
        if timing:
            ctx.set_timing(True)
            ctx.reset_timing()
        dts, t_enq = [], 0.0
        for _ in range(max(1, repeats)):
            fence()
            t0 = time.perf_counter()
            run_steps(steps)
            t_enq = time.perf_counter() - t0
            fence()
            dt_r = time.perf_counter() - t0
            if dist is not None:
                tt_ = torch.tensor([dt_r], dtype=torch.float64)
                dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
                dt_r = float(tt_.item())
            dts.append(dt_r)
            keep.clear()
        dt = float(np.median(dts))
        jl = (steps // G - 1) % depth                      # context of the region's last call; its step G - 1 is the last step
        res = dict(value=Qtot * steps / dt, ms_per_step=1e3 * dt / steps, host_enqueue_ms_per_step=1e3 * t_enq / steps,
                   repeats=len(dts), value_min=Qtot * steps / max(dts), value_max=Qtot * steps / min(dts),
                   ms_per_region=[1e3 * d for d in dts], steps=steps, group=G,
                   last_step=dict(d2=d2s[jl][G - 1], out=view(outs[jl], G - 1), gath=gath[jl]))
        if not timing:
            return res
        kern = {}
        for name, kid in (("edt_colbits", sc.K_EDT_COLBITS), ("edt_band", sc.K_EDT_BAND), ("moves", sc.K_MOVES), ("astar", sc.K_ASTAR),
                          ("gather", sc.K_GATHER), ("toppra", sc.K_TOPPRA), ("toppra_sample", sc.K_TOPPRA_SAMPLE)):
            ms, n = ctx.get_timing(kid)
            if n:
                kern[name] = {"ms_per_launch_on_context0": ms / n, "launches": n}
        ctx.set_timing(False)
        expansions = ctx.astar_last_expansions() // G      # mean over the steps of the last call on context 0
        out = view(outs[0], 0)
        st = out["status"].cpu().numpy()
        ln = out["len"].cpu().numpy()
        astar_ms = kern["astar"]["ms_per_launch_on_context0"]
        lastk = G - 1
        res.update(kernels=kern,
                   astar={"expansions_per_step_rank0": expansions,
                          "launch_ms_on_context0": astar_ms,
                          "expansions_per_s_whole_job": expansions * world * steps / dt,
                          "algorithmic_GBps_whole_job": 104 * expansions * world * steps / dt / 1e9,
                          "found": int((st == 0).sum()), "no_path": int((st == 1).sum()), "ring_overflow": int((st == 4).sum()),
                          "mean_path_len": float(ln[st == 0].mean()) if (st == 0).any() else 0.0},
                   _host=dict(occ=occ_h, s=s_h, g=g_h, out=out, st=st, d2=d2s[0][0], gath=gath[0],
                              lastk=lastk, occ_last=occ_hs[lastk], s_last=sg[lastk][0], g_last=sg[lastk][1], out_last=view(outs[0], lastk)))
        if with_toppra:
            res["toppra_ok"] = int((tp_last[0][0]["status"] == 0).sum())
            res["toppra_plans_per_call"] = G * Qloc
        return res

    if args.group <= 0:
        args.group = max(g for g in range(1, 33) if args.steps % g == 0)
    assert (args.group * Qtot) % world == 0
    main_run = run_map(args.map, args.steps, args.warmup, depth_max, group=args.group, repeats=args.repeats, timing=args.full)
    if args.dump_outputs and rank == 0:
        ls = main_run["last_step"]
        dump_outputs(args.dump_outputs, ls["d2"], ls["out"], ls["gath"], args.lmax,
                     gathered_rows=[(r * main_run["group"] + main_run["group"] - 1) * Qloc for r in range(world)], Qloc=Qloc)
    result = None
    if rank == 0:
        result = {
            "metric": "plans/sec (batched start-goal, 1024^2 grid)", "value": main_run["value"], "unit": "plans/s",
            "n_gpus": world, "steps": main_run["steps"], "warmup": args.warmup, "ms_per_step": main_run["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int32", "data": "synthetic",
            "repeats": main_run["repeats"], "value_is": "median over the repeats of the timed K-step region",
            "value_min": main_run["value_min"], "value_max": main_run["value_max"], "ms_per_region": main_run["ms_per_region"],
            "config": {"workload": f"{W}x{H} random-obstacle grids ({args.map}, one grid and one query block per step), EDT + A*, {Qloc} batched "
                                   f"queries per GPU and step, {main_run['group']} steps = {main_run['group'] * Qloc} queries per library call"
                                   + (", RCCL all-gather of paths" if use_gather else ""),
                       "queries_per_launch": main_run["group"] * Qloc,
                       "grid": [W, H], "map": args.map, "queries_per_gpu": Qloc, "queries_total": Qtot, "lmax": args.lmax,
                       "parallelism": f"query-sharded x{world}", "contexts_in_flight": depth_max, "steps_per_call": main_run["group"],
                       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "runtime default")},
            "host_enqueue_ms_per_step": main_run["host_enqueue_ms_per_step"],
        }

    def finish():
        if rank == 0:
            print(json.dumps(result))
        for c in ctxs:
            c.close()
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    if not args.full:
        finish()
        return

    seq_run = run_map(args.map, max(2, min(args.steps, 4)), 1, 1, repeats=args.repeats)   # one call per step, one stream
    qst = ctx.astar_debug_stats(Qloc)            # of seq_run's last call: expansions, popped entries, kilo-cycles, steps per query
    kc = np.sort(qst[2].astype(np.float64))
    per_query = {"kilocycles_p50": float(kc[len(kc) // 2]), "kilocycles_p99": float(kc[int(0.99 * (len(kc) - 1))]), "kilocycles_max": float(kc[-1]),
                 "steps_p50": float(np.median(qst[3])), "steps_max": int(qst[3].max()), "expansions_max": int(qst[0].max()),
                 "note": "one call of %d queries on one stream: in-kernel cycle count and dependent frontier steps of every search; the call ends with its longest search" % Qloc}
    others = {} if args.only_main_map else {f: run_map(f, args.steps, 1, depth_max, group=args.group) for f in FAMILIES if f != args.map}
    cfg2 = run_map(args.map, args.steps, 1, depth_max, with_toppra=True, group=args.group)
    occ_h, s_h, g_h, out, st = (main_run["_host"][k] for k in ("occ", "s", "g", "out", "st"))

    # ---- the gather must have left every rank with every rank's paths, in query order ----
    gather_info = None
    if use_gather:
        ga = main_run["_host"]["gath"]
        off = ga["offsets"].cpu().numpy()
        cells = ga["cells"].cpu().numpy()
        mine_p = out["path"].cpu().numpy()
        mine_l = out["len"].cpu().numpy()
        Gm = main_run["group"]
        m0 = rank * Gm * Qloc                      # step 0 of this rank's block in the gathered arrays
        ok = bool(np.array_equal(ga["len"].cpu().numpy()[m0:m0 + Qloc], mine_l) and np.array_equal(ga["status"].cpu().numpy()[m0:m0 + Qloc], st)
                  and np.array_equal(ga["cost"].cpu().numpy()[m0:m0 + Qloc], out["cost"].cpu().numpy()))
        for q in range(Qloc):
            if st[q] == 0:
                ok = ok and np.array_equal(cells[off[m0 + q]:off[m0 + q] + mine_l[q]], mine_p[q, :mine_l[q]])
        # the last step of this rank's block in the gathered arrays against that step's own results
        ol_ = main_run["_host"]["out_last"]
        l_l, l_s, l_p = ol_["len"].cpu().numpy(), ol_["status"].cpu().numpy(), ol_["path"].cpu().numpy()
        ml = m0 + (Gm - 1) * Qloc
        ok = ok and np.array_equal(ga["len"].cpu().numpy()[ml:ml + Qloc], l_l) and np.array_equal(ga["status"].cpu().numpy()[ml:ml + Qloc], l_s)
        for q in range(0, Qloc, 17):
            if l_s[q] == 0:
                ok = ok and np.array_equal(cells[off[ml + q]:off[ml + q] + l_l[q]], l_p[q, :l_l[q]])
        # paths of ANOTHER rank's block: replan a sample of its queries here (query i is the same on any rank) and compare
        checked_other = 0
        if world > 1:
            r2_ = (rank + 1) % world
            o0, o1 = shard.rank_range(Qtot, world, r2_)
            ns = min(64, o1 - o0)
            so, go = synth.queries(main_run["_host"]["d2"].cpu().numpy() >= 1, ns, first=o0)
            oo = ctx.astar_batch(main_run["_host"]["d2"], torch.from_numpy(so).to(dev), torch.from_numpy(go).to(dev), Lmax=args.lmax)
            ctx.synchronize()
            op, ol, ost = oo["path"].cpu().numpy(), oo["len"].cpu().numpy(), oo["status"].cpu().numpy()
            gl, gs = ga["len"].cpu().numpy(), ga["status"].cpu().numpy()
            n0 = r2_ * Gm * Qloc                    # step 0 of that rank's block
            for q in range(ns):
                ok = ok and gs[n0 + q] == ost[q] and gl[n0 + q] == ol[q]
                if ost[q] == 0:
                    ok = ok and np.array_equal(cells[off[n0 + q]:off[n0 + q] + ol[q]], op[q, :ol[q]])
            checked_other = ns
        okt = torch.tensor([1 if ok else 0], dtype=torch.int32)
        if dist is not None:
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        assert int(okt.item()) == 1, "gather of result paths is inconsistent"
        gather_info = {"entry_point": "sc_allgather_paths (pack kernel -> one ncclAllGather over RCCL -> unpack kernel)",
                       "exchanges": "one per library call (all steps of the call)",
                       "bytes_received_per_rank_per_step": ctx.allgather_last_bytes() // Gm,
                       "fixed_stride_bytes_per_rank_per_step": Qtot * (args.lmax + 3) * 4,
                       "cells_per_rank_capacity_per_step": cap_cells, "truncated": int(ga["truncated"][0]),
                       "paths_checked": "own block (first step cell for cell, last step sampled)" + (f"; {checked_other} queries of rank {(rank + 1) % world}'s block replanned here and compared" if world > 1 else ""),
                       "consistent_on_all_ranks": True}

    if rank == 0:
        result.update({
            "value_depth1": seq_run["value"], "ms_per_step_depth1": seq_run["ms_per_step"],
            "value_depth1_is": f"one library call per step ({Qloc} queries per launch) on one stream: what BASELINE configs[1] literally describes",
            "per_query_depth1": per_query,
            "kernels": main_run["kernels"], "astar": main_run["astar"],
            "other_maps": {f: {"value": r["value"], "ms_per_step": r["ms_per_step"],
                               "expansions_per_step_rank0": r["astar"]["expansions_per_step_rank0"]} for f, r in others.items()},
            "configs2": {"workload": f"the same step + TOPP-RA (6 joints, 200 stages, sampled at 20 ms) of {Qloc} plans per GPU",
                         "value": cfg2["value"], "ms_per_step": cfg2["ms_per_step"], "toppra_ok": cfg2.get("toppra_ok"),
                         "toppra_plans_per_call": cfg2.get("toppra_plans_per_call"),
                         "note": "the plans of a call's steps are handed over in one sc_toppra_hermite_batch call, as its queries are in one sc_astar_batch_multi call; toppra_ok counts the whole call"},
        })
        if gather_info:
            result["gather"] = gather_info

    # ---- roofline leg: EDT on a batch of grids (rank 0 only, N = 1 semantics) ----
    if rank == 0:
        def edt_leg(family, Wl, Hl, B):
            grids = torch.from_numpy(np.stack([make_grid(family, Wl, Hl, seed=synth.SEED_GRID + i) for i in range(B)])).to(dev)
            d2b = torch.empty((B, Hl, Wl), dtype=torch.int32, device=dev)
            # HIP events on the stream the kernels are launched on: `iters` EDTs back to back inside ONE bracket, so the
            # few microseconds an event pair costs are not charged to every 70 us launch
            ts = torch.cuda.Stream(device=dev)
            ctx.set_stream(ts.cuda_stream)
            for _ in range(3):
                ctx.edt(grids, out=d2b)
                ctx.synchronize()       # a context adapts to maps of open space when it is synchronised
            ts.synchronize()
            iters = 20
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            for _ in range(iters):
                ctx.edt(grids, out=d2b)
            e1.record(ts)
            ts.synchronize()
            per_launch_ms = e0.elapsed_time(e1) / iters
            # split by kernel (in-library event pair around every launch; adds event overhead, informational)
            ctx.set_timing(True)
            ctx.reset_timing()
            for _ in range(iters):
                ctx.edt(grids, out=d2b)
            ts.synchronize()
            ms_a, _ = ctx.get_timing(sc.K_EDT_COLBITS)
            ms_b, _ = ctx.get_timing(sc.K_EDT_BAND)
            ctx.set_timing(False)
            ctx.use_own_stream()
            alg_bytes = EDT_BYTES_PER_CELL * B * Wl * Hl
            achieved = alg_bytes / (per_launch_ms * 1e-3) / 1e9
            del grids, d2b
            return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                    "kernel": ("edt_colbits_kernel + edt_band_g8_kernel (one EDT = both launches)" if Wl <= 1024 else
                               "edt_colbits_kernel + edt_updown_kernel + edt_band_wide_kernel (one EDT = the three launches)"),
                    "workload": f"EDT of {B} x {Wl}x{Hl} {family} grids per launch pair",
                    "algorithmic_bytes_per_launch": alg_bytes, "ms_per_launch": per_launch_ms,
                    "timing": f"HIP events around {iters} back-to-back EDTs on the launch stream",
                    "ms_colbits_bracketed": ms_a / iters, "ms_band_bracketed": ms_b / iters}

        B = args.edt_batch
        legs = {fam: edt_leg(fam, W, H, B) for fam in FAMILIES}
        result["roofline"] = legs[args.map]
        # measured device-to-device copy bandwidth on this box (256 MiB read + 256 MiB written per copy), for scale
        src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        torch.cuda.synchronize()
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(20):
            dst.copy_(src)
        c1.record()
        torch.cuda.synchronize()
        copy_gbs = 2 * src.numel() * 20 / (c0.elapsed_time(c1) * 1e-3) / 1e9
        result["roofline"]["measured_copy_GBps"] = copy_gbs
        result["roofline"]["frac_of_measured_copy"] = result["roofline"]["achieved"] / copy_gbs
        del src, dst
        # HBM traffic of the same workload from the PMC counters: collected by rocprofv3 in separate passes (the counters
        # cannot be read from inside this process), kept under profiles/ with the command that made them
        tpath = os.path.join(ROOT, "profiles", "edt_traffic.json")
        if os.path.exists(tpath) and (W, H, args.edt_batch) == (1024, 1024, 64):
            try:
                tj = json.load(open(tpath))
                result["roofline"]["traffic"] = tj.get(args.map, {}).get("hbm_bytes_per_launch")
                result["roofline"]["traffic_source"] = "profiles/edt_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; not measured in this run)"
            except Exception:
                pass
        keys = ("achieved", "frac", "ms_per_launch", "ms_colbits_bracketed", "ms_band_bracketed")
        result["roofline_other_maps"] = {k: {kk: v[kk] for kk in keys} for k, v in legs.items() if k != args.map}
        if not args.only_main_map:
            open_leg = edt_leg("open", W, H, B)
            result["roofline_other_maps"]["open"] = {kk: open_leg[kk] for kk in keys}
            result["roofline_other_maps"]["open"]["note"] = ("2e-5 of the cells occupied: rows the packed cascade cannot settle (distances beyond 175 "
                                                             "columns) go through the site search; bound by instruction issue, not HBM (DESIGN.md 4.1)")
        if (W, H) == (1024, 1024):   # BASELINE configs[3]'s grid: the same number of cells per launch pair
            result["roofline_4096"] = {fam: {kk: v[kk] for kk in keys + ("workload",)}
                                       for fam, v in ((f, edt_leg(f, 4096, 4096, max(1, B // 16))) for f in (("salt20", "blocks") if args.only_main_map else ("salt20", "blocks", "open")))}
            # the same kernels on a batch sized for HBM rather than for parity with the 1024^2 leg's byte count: 16 grids = 1.3 GB
            # per launch (a persistent workgroup then runs 16 row groups instead of 4: pipeline fill and launch gaps amortised)
            if B >= 64:
                v16 = edt_leg("salt20", 4096, 4096, 16)
                result["roofline_4096"]["salt20_16_grids"] = {kk: v16[kk] for kk in keys + ("workload",)}

        # ---- TOPP-RA leg (BASELINE configs[2]: 1k plans, 6-DOF, 200 waypoints): the kernels alone ----
        P, dof, N = 1024, 6, 200
        pl = synth.toppra_plans(P, dof=dof)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        targs = (tt(pl["p0"]), tt(pl["p1"]), tt(pl["v0"]), tt(pl["v1"]), tt(-pl["vlim"]), tt(pl["vlim"]), tt(-pl["alim"]), tt(pl["alim"]))
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        for _ in range(2):
            tp = ctx.toppra(*targs, N=N)
        torch.cuda.synchronize()
        ctx.set_timing(True)
        ctx.reset_timing()
        for _ in range(10):
            tp = ctx.toppra(*targs, N=N)
            smp = ctx.toppra_sample(targs[0], targs[1], targs[2], targs[3], tp["x"], tp["t"], 0.02, 512)
        torch.cuda.synchronize()
        ms_t, _ = ctx.get_timing(sc.K_TOPPRA)
        ms_s, _ = ctx.get_timing(sc.K_TOPPRA_SAMPLE)
        ctx.set_timing(False)
        ok_plans = int((tp["status"] == 0).sum())
        tbytes = 128 * P * (N + 1)  # 128 B per (plan, stage) at dof 6
        result["toppra"] = {"plans": P, "dof": dof, "stages": N, "ok": ok_plans, "ms_sweep": ms_t / 10, "ms_sample": ms_s / 10,
                            "plans_per_s": P / ((ms_t + ms_s) / 10 * 1e-3), "algorithmic_GBps": tbytes / (ms_t / 10 * 1e-3) / 1e9,
                            "hbm_frac": tbytes / (ms_t / 10 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "note": "bound by instruction issue (two dependent 200-stage sweeps per plan and 4 dof^2 row pairs per stage), not by HBM"}

    # ---- dynamic-obstacle replan stream (BASELINE configs[4]), N = 1 only: reported, not part of `value` ----
    if rank == 0 and world == 1 and args.replan_frames > 0:
        rects = synth.block_rects(W, H)
        occ0 = synth.raster_rects(rects, W, H)
        frames = [rects]
        for f in range(1, args.replan_frames + 2):
            frames.append(synth.move_rects(frames[-1], f, W, H))
        frames_dev = [torch.from_numpy(r).to(dev) for r in frames]
        occ_dev = torch.empty((H, W), dtype=torch.uint8, device=dev)
        replan = {"map": "blocks (256 rectangles, 32 moved by <= 2 cells per frame)", "frames": args.replan_frames}
        for Qf in (8192, 8192 // 8):
            sf, gf = synth.queries(occ0 == 0, Qf)
            sfd, gfd = torch.from_numpy(sf).to(dev), torch.from_numpy(gf).to(dev)

            def frame(i):
                ctx.occ_from_rects(frames_dev[i], W, H, out=occ_dev)
                d2f = ctx.edt(occ_dev)
                return ctx.astar_batch(d2f, sfd, gfd, Lmax=args.lmax)
            frame(0)
            frame(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.replan_frames):
                of = frame(2 + i)
                torch.cuda.synchronize()            # a frame's paths are due before the next frame arrives
            ms = (time.perf_counter() - t0) / args.replan_frames * 1e3
            replan[f"q{Qf}"] = {"queries_per_frame": Qf, "ms_per_frame": ms, "frames_per_s": 1e3 / ms, "meets_30hz": ms < 1e3 / 30,
                                "found_last_frame": int((of["status"] == 0).sum())}
        replan["note"] = ("per frame: rectangle list -> occupancy grid, full exact EDT, legal moves, batched A*, synchronised; "
                          "q8192 = the whole 8k-query frame on ONE GPU, q1024 = one GPU's share when 8 GPUs split the frame")
        result["replan_stream"] = replan

    # ---- BASELINE configs[3], one GPU's share: 4096^2 grid, 8192 of the 64k queries (rank 0's block), N = 1 only, with the
    # gather of the result paths in the loop: pack -> (ncclAllGather when a communicator exists: SC_BENCH_FORCE_DIST=1) -> unpack
    if rank == 0 and world == 1 and not args.only_main_map:
        W4 = H4 = 4096
        occ4 = torch.from_numpy(make_grid(args.map, W4, H4)).to(dev)
        d4 = ctx.edt(occ4)
        torch.cuda.synchronize()
        Q4 = 8192
        s4, g4 = synth.queries(d4.cpu().numpy() >= 1, Q4)            # queries 0 .. 8191 of the 64k (rank 0 of 8)
        s4d, g4d = torch.from_numpy(s4).to(dev), torch.from_numpy(g4).to(dev)
        L4 = 4 * args.lmax
        o4 = ctx.astar_batch(ctx.edt(occ4), s4d, g4d, Lmax=L4)       # warm-up (scratch allocation)
        torch.cuda.synchronize()
        # message capacity from the measured path lengths (mean ~2-3 k cells of Lmax 16 k) with a quarter of headroom, not
        # from Lmax: the gather then moves what the paths hold instead of Q * Lmax / 4 cells per rank
        eff4 = torch.where(o4["status"] == 0, o4["len"], torch.zeros_like(o4["len"]))
        cells4 = int(eff4.sum())
        cap4 = int(1.25 * cells4) + 1024
        words4 = int(sc.lib().sc_gather_msg_words(Q4, 1, cap4))
        msg4 = torch.empty(words4, dtype=torch.int32, device=dev)
        gb4 = None

        def gather4(o):
            if use_gather:
                return ctx.allgather_paths(o, Q4, cap4, bufs=gb4)
            ctx.gather_pack(o, Q4, 1, 0, cap4, msg=msg4)
            return ctx.gather_unpack(msg4, 1, Q4, L4, cap4)
        gb4 = gather4(o4) if use_gather else None
        torch.cuda.synchronize()
        ctx.set_timing(True)
        ctx.reset_timing()
        t0 = time.perf_counter()
        o4 = ctx.astar_batch(ctx.edt(occ4), s4d, g4d, Lmax=L4)
        ga4 = gather4(o4)
        torch.cuda.synchronize()
        dt4 = time.perf_counter() - t0
        ms_g4, n_g4 = ctx.get_timing(sc.K_GATHER)
        ms_a4, _ = ctx.get_timing(sc.K_ASTAR)
        ms_e4 = ctx.get_timing(sc.K_EDT_COLBITS)[0] + ctx.get_timing(sc.K_EDT_BAND)[0]
        ctx.set_timing(False)
        ex4 = ctx.astar_last_expansions()
        st4 = o4["status"].cpu().numpy()
        ln4 = o4["len"].cpu().numpy()
        # the gathered result against the call's own outputs: lengths, statuses, offsets, a sample of the paths cell for cell
        off4 = ga4["offsets"].cpu().numpy()
        ok4 = bool(np.array_equal(ga4["len"].cpu().numpy(), ln4) and np.array_equal(ga4["status"].cpu().numpy(), st4) and int(ga4["truncated"][0]) == 0
                   and off4[-1] == int(np.where(st4 == 0, ln4, 0).sum()))
        c4 = ga4["cells"].cpu().numpy()
        p4 = o4["path"][::64].cpu().numpy()
        for qi, q in enumerate(range(0, Q4, 64)):
            if st4[q] == 0:
                ok4 = ok4 and np.array_equal(c4[off4[q]:off4[q] + ln4[q]], p4[qi, :ln4[q]])
        result["config3_one_gpu_share"] = {"workload": f"{W4}x{H4} {args.map} grid, EDT + A* + gather of the paths, {Q4} queries (one GPU's block of the 64k), Lmax {L4}",
                                           "ms": dt4 * 1e3, "plans_per_s": Q4 / dt4, "expansions": int(ex4), "G_expansions_per_s": ex4 / dt4 / 1e9,
                                           "ms_edt": ms_e4, "ms_astar": ms_a4,
                                           "found": int((st4 == 0).sum()), "truncated": int((st4 == 3).sum()), "ring_overflow": int((st4 == 4).sum()),
                                           "mean_path_cells": float(ln4[st4 == 0].mean()) if (st4 == 0).any() else 0.0,
                                           "gather": {"transport": "ncclAllGather (RCCL, world 1)" if use_gather else "none (sc_gather_pack -> sc_gather_unpack on the same message)",
                                                      "cap_cells": cap4, "cap_cells_rule": "1.25 x the cells of the previous batch's paths + 1024",
                                                      "message_bytes_per_rank": 4 * words4, "bytes_received_per_rank_at_8_ranks": 8 * 4 * words4,
                                                      "fixed_stride_bytes_per_rank": Q4 * (L4 + 3) * 4,
                                                      "ms_pack_and_unpack": ms_g4, "launch_groups": n_g4, "gathered_equals_own_results": ok4},
                                           "note": "the 8-GPU job gathers 8 such blocks with sc_allgather_paths; not measured on more than one GPU"}
        assert ok4, "config3: gathered paths differ from the call's own results"
        del occ4, d4, o4, ga4, msg4

    # ---- what follows the planner in the reference (examples/zmq_test.cpp:66-93), batched: SURVEY 8f rows 1-2 ----
    # the step's own A* paths -> 16 waypoints each -> from_path -> arclength -> TOPP-RA along the arclength -> sampling at
    # 20 ms -> resample (nudge) + curvature; reported beside the headline, not part of `value`
    if rank == 0 and world == 1 and not args.only_main_map:
        from sea_current_amd import pipeline
        ln_h = out["len"].cpu().numpy()
        sel = (st == 0) & (ln_h >= 64)
        wp_h = pipeline.waypoints_from_cells(out["path"].cpu().numpy()[sel], ln_h[sel], W, n_wp=16, cell_m=0.05)
        wp_d = torch.from_numpy(wp_h).to(dev)
        sm = pipeline.smooth_batch(ctx, wp_d)                    # warm-up; fixes the samples reserved per path
        ctx.synchronize()
        ctx.reset_timing(); ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(5):
            sm = pipeline.smooth_batch(ctx, wp_d, max_len=sm["max_len"])
        ctx.synchronize()
        t_sm = (time.perf_counter() - t0) / 5
        stage_ms = {name: ctx.get_timing(kid)[0] / 5 for name, kid in (("from_path", sc.K_BEZIER), ("arclength", sc.K_ARCLENGTH), ("toppra", sc.K_TOPPRA),
                                                                        ("sampling", sc.K_TOPPRA_SAMPLE), ("resample", sc.K_RESAMPLE))}
        ctx.set_timing(False)
        Psm, Msm = int(wp_h.shape[0]), int(sm["pos"].shape[0])
        # algorithmic bytes: waypoints in; control points, arclength tables, profile knots, then 9 float32 per sample out
        # (pos, vel, acc, point x / y, parameter, segment, curvature, + the nudged position read back)
        sm_bytes = Psm * (16 * 8 + 15 * (32 + 404) + 101 * 16) + Msm * 36
        result["smoothing"] = {"workload": f"{Psm} of the step's A* paths (found, >= 64 cells), 16 waypoints each (0.05 m cells): from_path -> arclength (GL-32, 100 "
                                           "subdivisions per segment) -> TOPP-RA along the arclength (1 dof, 100 stages, v <= 1 m/s, |a| <= 0.5 m/s^2) -> sampling at "
                                           "20 ms -> resample with nudge (degree-9 Chebyshev fit per segment) + curvature",
                               "paths": Psm, "samples": Msm, "ms_per_batch": t_sm * 1e3, "paths_per_s": Psm / t_sm, "samples_per_s": Msm / t_sm,
                               "ms_kernels": stage_ms, "ms_kernels_sum": sum(stage_ms.values()),
                               "algorithmic_GBps": sm_bytes / (sum(stage_ms.values()) * 1e-3) / 1e9,
                               "hbm_frac": sm_bytes / (sum(stage_ms.values()) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                               "resample_ok": int((sm["resample_status"] == 0).sum()), "toppra_ok": int((sm["toppra_status"] == 0).sum()),
                               "note": "ms_per_batch is host wall time for the five library calls and the torch bookkeeping between them; fp64 / fp32 as the reference; "
                                       "bound by the dependent chains inside a path (TOPP-RA sweeps, the nudge replay, the fit), not by HBM"}
        if not args.no_cpu_baseline:
            from oracle import oracle  # checker / baseline only
            oracle.build()
            t0 = time.perf_counter()
            refs = [oracle.smooth_one(wp_h[b]) for b in range(min(32, Psm))]
            t_c = time.perf_counter() - t0
            offs, lens_g = sm["offsets"].cpu().numpy(), sm["length"].cpu().numpy()
            pts_g = sm["pts"].cpu().numpy()
            okp = all(abs(int(lens_g[b]) - r["length"]) <= 1 and (int(lens_g[b]) != r["length"] or float(np.abs(pts_g[offs[b]:offs[b + 1]] - r["pts"]).max()) < 2e-4)
                      for b, r in enumerate(refs))
            result["smoothing"]["cpu"] = {"paths_per_s": len(refs) / t_c, "cores": 1, "kind": "port", "sample": f"the first {len(refs)} paths of the batch",
                                          "gpu_matches_cpu_on_sample": bool(okp)}

    # ---- the reference's own planner, FMT* over Halton samples, batched: reported, not part of `value` ----
    if rank == 0 and world == 1 and not args.only_main_map:
        fl, fo = synth.polygon_world(14, 5.0)
        fs = synth.free_samples(1000, 5.0, fl, fo)
        frng = np.random.default_rng(0xF37)
        Qf = 1024
        fst, fgo = fs[frng.integers(0, fs.shape[0], Qf)], fs[frng.integers(0, fs.shape[0], Qf)]
        td = lambda a_: torch.from_numpy(np.ascontiguousarray(a_, np.float32)).to(dev)
        fsd, fstd, fgod, fld = td(fs), td(fst), td(fgo), td(fl)
        fo_ = ctx.fmt_star(fsd, fstd, fgod, 0.9, fld, Lmax=128)
        ctx.synchronize()
        ctx.reset_timing(); ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(3):
            fo_ = ctx.fmt_star(fsd, fstd, fgod, 0.9, fld, Lmax=128)
        ctx.synchronize()
        t_f = (time.perf_counter() - t0) / 3
        ms_f = ctx.get_timing(sc.K_FMT)[0] / 3
        ctx.set_timing(False)
        fstat = fo_["status"].cpu().numpy()
        result["fmt_star"] = {"workload": f"{Qf} start-goal pairs over 1000 Halton samples of a 10 x 10 world with 14 convex polygons ({fl.shape[0]} edges), "
                                          "connection radius 0.9: fast_marching_trees (sea_current.hpp:1339-1407), one wavefront per query",
                              "queries": Qf, "ms_per_batch": t_f * 1e3, "ms_kernel": ms_f, "plans_per_s": Qf / t_f, "found": int((fstat == 0).sum()),
                              "note": "the reference's planner restated (parity vs the reference unpinned: it holds no recorded FMT* output); per query "
                                      "the tree grows over up to 1002 samples with a segment-vs-every-edge test per candidate connection"}
        if not args.no_cpu_baseline:
            from oracle import oracle  # checker / baseline only
            oracle.build()
            t0 = time.perf_counter()
            frefs = [oracle.fmt_star(fs, fst[q_], fgo[q_], 0.9, fl, Lmax=128) for q_ in range(32)]
            t_c = time.perf_counter() - t0
            fp_, fl_, fc_ = fo_["path"].cpu().numpy(), fo_["len"].cpu().numpy(), fo_["cost"].cpu().numpy()
            okf = all(fstat[q_] == r_["status"] and (r_["status"] != 0 or (fl_[q_] == r_["len"] and fc_[q_] == np.float32(r_["cost"])
                                                                           and np.array_equal(fp_[q_, :r_["len"]], r_["path"]))) for q_, r_ in enumerate(frefs))
            result["fmt_star"]["cpu"] = {"plans_per_s": len(frefs) / t_c, "cores": 1, "kind": "port", "sample": "the first 32 queries of the batch",
                                         "gpu_matches_cpu_on_sample": bool(okf)}

    # ---- CPU baseline leg (rank 0, N = 1 only) ----
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import oracle  # checker / baseline only, never the measured product
        oracle.build()
        # gpurun boxes give one GPU a 16-core share of the host; never oversubscribe it
        cores = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
        t0 = time.perf_counter()
        d2_ref = oracle.edt(occ_h)
        t_edt = time.perf_counter() - t0
        # bounded sample: whole query sets of the same workload (set k = queries k*Q .. (k+1)*Q-1 of the same
        # generator; set 0 is exactly what the GPU just planned) until ~cpu-seconds of A* work have run
        trav = d2_ref >= 1
        t_as, nq, nexp, ref0 = 0.0, 0, 0, None
        k = 0
        while t_as < args.cpu_seconds and k < 64:
            sk, gk = (s_h, g_h) if k == 0 else synth.queries(trav, Qloc, first=k * Qloc)
            t0 = time.perf_counter()
            ref = oracle.astar_batch(d2_ref, sk, gk, Lmax=args.lmax, nthreads=cores)
            t_as += time.perf_counter() - t0
            nq += Qloc
            nexp += int(ref["expanded"].sum())
            if k == 0:
                ref0 = ref
            k += 1
        # single-thread figure (the reference is single-threaded): the first 128 queries of set 0
        t0 = time.perf_counter()
        oracle.astar_batch(d2_ref, s_h[:128], g_h[:128], Lmax=args.lmax, nthreads=1)
        t_1 = time.perf_counter() - t0
        # parity spot-check of what was just timed on the GPU (set 0 = the same queries)
        pth = out["path"].cpu().numpy()
        ok = bool(np.array_equal(ref0["status"], st) and np.array_equal(ref0["cost"], out["cost"].cpu().numpy())
                  and all(np.array_equal(pth[q, :ref0["len"][q]], ref0["path"][q, :ref0["len"][q]]) for q in range(Qloc)))
        # ... and of a step other than step 0 of the same library call: its own grid and query block
        hl = main_run["_host"]
        ok_last = None
        if hl["lastk"] > 0:
            d2_l = oracle.edt(hl["occ_last"])
            ref_l = oracle.astar_batch(d2_l, hl["s_last"], hl["g_last"], Lmax=args.lmax, nthreads=cores)
            o_l = hl["out_last"]
            p_l = o_l["path"].cpu().numpy()
            ok_last = bool(np.array_equal(ref_l["status"], o_l["status"].cpu().numpy()) and np.array_equal(ref_l["cost"], o_l["cost"].cpu().numpy())
                           and all(np.array_equal(p_l[q, :ref_l["len"][q]], ref_l["path"][q, :ref_l["len"][q]]) for q in range(Qloc)))
        result["cpu_baseline"] = {"value": nq / (k * t_edt + t_as), "unit": "plans/s", "cores": cores, "kind": "port",
                                  "sample": f"{k} query sets of {Qloc} (exact EDT of the grid per set: {t_edt:.3f} s, 1 thread; "
                                            f"A* on {cores} threads: {t_as:.1f} s in total); build's own C restatement -- "
                                            "the reference has no grid path",
                                  "edt_seconds_1thread": t_edt, "astar_expansions": nexp,
                                  "single_thread_value": 128 / (t_edt * 128 / Qloc + t_1),
                                  "gpu_matches_cpu_on_sample": ok,
                                  "gpu_matches_cpu_on_step": {"step_of_the_call": hl["lastk"], "matches": ok_last}}
    finish()


if __name__ == "__main__":
    main()
