#!/usr/bin/env python3
"""bench.py — events/sec through divide_rounds + decide_fame (BASELINE.json metric).

One "step" = sw_rewind + sw_divide_rounds + sw_decide_fame through the C-ABI over one synthetic
hashgraph whose events are ALREADY resident in HBM (sw_append_events is ingest, mirrors
Node.add_event, outside the timed region of `value`; `value_end_to_end` includes it, see below).
Workload at N=1: BASELINE.json configs[2] — 256 members, 1M events, uniform gossip
(SURVEY.md §8d generator), seed 3.

--gpus N measures TWO things in one run and says which one is `value` (`"scaling"`):
  * N INDEPENDENT replicas of the workload (one hashgraph per GPU, different seeds) — `value`, `"scaling":
    "weak-replicas"`, the default: what a deployment has (every member holds its own view);
  * ONE hashgraph over the N GPUs — `value_strong` (with `--split strong` it becomes `value`, `"scaling": "strong"`):
    py-swirld_amd/partition.py StrongSplit — the can_see sweep split by event ranges (every rank sweeps its
    range from a halo, no communication), the ranges broadcast as int32 rows over RCCL while the round loop
    (replicated: one chain of dependent iterations) already works on the ranges that arrived, and the
    elections candidate-partitioned with one all-reduce.  DESIGN.md §8 says why this cannot reach north_star's
    >= 6x at 8 GPUs; this number is the evidence.

Extra fields of the JSON line:
  value_end_to_end  events/s from "SoA arrays in host memory" to "round[N], witness table, famous,
                    new_c back in host memory" (SURVEY.md §8d Timing): sw_reset + sw_append_events +
                    sw_divide_rounds + sw_decide_fame + getters, on a context whose device storage is
                    already allocated.  PCIe-inclusive; never `value`.
  value_with_order  events/s of divide_rounds + decide_fame + find_order (N1, swirld.py:280-311): N / (ms_per_step +
                    find_order_ms); find_order is outside the metric and timed once, after the profiled pass.
  roofline          the kernel with the largest total time, plus a `kernels` table (every family of
                    the path: algorithmic bytes per launch per SURVEY.md §8d, average launch duration
                    measured live with hipEvents, counter-measured HBM bytes per launch from the
                    same-commit rocprofv3 --pmc passes in profiles/traffic.json) and the whole-path
                    algorithmic rate.
  cpu_baseline      the C oracle (kind "port") on one host core over a bounded sample; `reference_python` next to it
                    is the unmodified reference itself: timed IN THIS RUN on a short prefix when its source tree is
                    reachable (`--reference-path`, default /root/reference: the authoring container), else the
                    committed measurement of profiles/reference_python_timing.json (`same_run` says which).

A plain run (no `--full`) sets up, warms up, times the `--steps` steps and prints the line: `value` / `ms_per_step`
and the `config` of the workload.  Everything else above — value_end_to_end, value_with_order / find_order, roofline,
cpu_baseline, the concurrent-contexts figure and the one-hashgraph split (unless `--split strong` or `--emulate-parts`
asks for it) — takes runs of its own and is measured only with `--full`; without it those fields are null.

--dump-outputs DIR writes what the last timed step computed, as a caller of the path receives it, to DIR/<name>.npy
(float64, 64 MB at most; larger tables as a fixed, seeded sample of rows, with the row indices next to them):
new_c, rounds, witnesses, famous and sampled can_see rows.  The inputs depend only on the arguments, so two builds can
be compared output for output.

Prints ONE JSON line on rank 0.
"""
import argparse
import importlib
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_GBPS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md); ~6300 achievable


def algorithmic_bytes(n, counters, n_events):
    """divide_rounds 12n + n^2/8 + 24 per non-root event;
    decide_fame V*(4n + n^2/8) + P2*n/8."""
    dr = (n_events - n) * (12 * n + n * n // 8 + 24)
    df = counters["voter_evals"] * (4 * n + n * n // 8) + counters["majority_evals"] * (n // 8)
    return dr, df


def npad_of(n):
    return ((n + 63) // 64) * 64


def kernels_sha256():
    """SHA-256 of the kernel source (kernels.hip.h + order.hip.h): what a counter measurement is valid for"""
    import hashlib
    h = hashlib.sha256()
    for name in ("kernels.hip.h", "order.hip.h"):
        with open(os.path.join(ROOT, "py-swirld_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def workload_key(n, N, mode, p0=0.0, p1=0.0):
    return "%dx%dx%d" % (n, N, mode) + (("_%g_%g" % (p0, p1)) if mode else "")


def load_traffic(key):
    """profiles/traffic.json: per WORKLOAD ("<members>x<events>x<generator mode>") the HBM bytes per launch of every
    kernel family from rocprofv3 --pmc passes (FETCH_SIZE doubled + WRITE_SIZE, separate passes) and rocprofv3's own
    average launch durations — measured by profiles/collect_traffic.py, not by this run.  Nothing is quoted for a
    workload the file does not hold, nor from a file measured on other kernel source (`stale`: the file carries the
    SHA-256 of kernels.hip.h + order.hip.h).  Returns (bytes per launch, ms per pass by rocprofv3's plain kernel trace of
    the bench command, commit, command, stale)."""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        t = json.load(open(tpath))
    except Exception:
        return {}, {}, None, None, True
    stale = t.get("kernels_sha256") != kernels_sha256()
    w = t.get("workloads", {}).get(key)
    if stale or not w:
        return {}, {}, (w or {}).get("commit"), None, stale
    return w.get("kernels", {}), w.get("ms_per_pass", {}), w.get("commit"), w.get("workload"), False


def time_python_reference(ref_path, n, stream, events):
    """The unmodified pure-Python reference on the first `events` events of this run's stream, one core, stdout
    suppressed (BASELINE.md §3 protocol), through the test harness that imports it (tests/refharness.py)."""
    if not os.path.isfile(os.path.join(ref_path, "swirld.py")):
        return None
    try:
        sys.path[:0] = [os.path.join(ROOT, "tests")]
        os.environ.setdefault("SWIRLD_REFERENCE_PATH", ref_path)
        import refharness
        M = min(events, len(stream[0]))
        ref = refharness.RefRun(n)
        ref.append(*[a[:M] for a in stream])
        t0 = time.perf_counter()
        ref.divide_rounds(0, M)
        ref.decide_fame()
        dt = time.perf_counter() - t0
        return {"events_per_s": round(M / dt, 1), "events": M, "members": n, "cores": 1, "seconds": round(dt, 2),
                "same_run": True, "where": "this run (reference tree at %s)" % ref_path,
                "note": "prefix-sampled: the cost per event still rises over the first rounds (622 / 433 / 265 events/s on 4 k / 8 k / 15 k "
                        "events at 256 members in the authoring container), so a longer prefix reads lower"}
    except Exception as exc:  # noqa: BLE001
        return {"same_run": False, "error": repr(exc)}


def guarded(fn, timeout_s, on_timeout, linger_s=1.0):
    """fn() on the calling thread.  If it has not returned after timeout_s seconds (0 = no limit), on_timeout() runs on a timer
    thread and the PROCESS ends with status 0 `linger_s` later — for work that may block for ever inside a collective (the
    thread cannot be interrupted, the process can): what had to be printed is printed by on_timeout."""
    if timeout_s <= 0:
        return fn()

    def bail():
        try:
            on_timeout()
            sys.stdout.flush()
        finally:
            time.sleep(linger_s)   # (rank 0's line is out before any process of the job goes away)
            os._exit(0)
    timer = threading.Timer(timeout_s, bail)
    timer.daemon = True
    timer.start()
    try:
        return fn()
    finally:
        timer.cancel()


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, h, new_c, seed):
    """The last timed step's results, as a caller of divide_rounds + decide_fame reads them back, as float64 .npy files.
    Event-indexed tables larger than their share of DUMP_CAP_BYTES are sampled: fixed, seeded row blocks, sorted,
    whose indices are written as <name>_rows.npy."""
    os.makedirs(out_dir, exist_ok=True)
    N, n = h.num_events, h.n
    rng = np.random.default_rng(seed)
    share = DUMP_CAP_BYTES // 4          # rounds / can_see / witnesses / famous get a quarter each; new_c is tiny

    def rows_within(n_rows, row_bytes):
        if n_rows * row_bytes <= share:
            return None
        blk = 256
        k = max(1, share // (row_bytes * blk))
        starts = np.sort(rng.choice(max(1, n_rows // blk), size=min(k, max(1, n_rows // blk)), replace=False)) * blk
        return np.unique(np.concatenate([np.arange(s, min(n_rows, s + blk)) for s in starts]))

    def save(name, a, rows=None):
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, np.float64))
        if rows is not None:
            np.save(os.path.join(out_dir, name + "_rows.npy"), rows.astype(np.float64))

    save("new_c", np.asarray(list(new_c), np.int64))
    rows = rows_within(N, 8)
    save("rounds", h.rounds() if rows is None else h.rounds()[rows], rows)
    wit, fam = h.witnesses(), h.famous()
    rows = rows_within(len(wit), 8 * n)
    save("witnesses", wit if rows is None else wit[rows], rows)
    save("famous", fam if rows is None else fam[rows], rows)
    rows = rows_within(N, 8 * n)
    if rows is None:
        save("can_see", h.can_see())
    else:
        starts = rows[np.r_[True, np.diff(rows) > 1]]
        ends = rows[np.r_[np.diff(rows) > 1, True]] + 1
        save("can_see", np.concatenate([h.can_see(int(a), int(b - a)) for a, b in zip(starts, ends)]), rows)


def strong_section(args, pkg, part_mod, rep, torch, rank, local_rank, world, n, N, stream, new_c, barrier):
    """The one-hashgraph split, timed (world > 1) or emulated with several contexts on one device (--emulate-parts)."""
    strong = None
    if world > 1 and npad_of(n) <= 256:
        import torch.distributed as dist

        dev = torch.device("cuda", local_rank)
        s_stream = pkg.synth_hashgraph(n, N, args.seed, args.mode, args.p0, args.p1)
        hs = pkg.Hashgraph(n, device=local_rank)
        hs.reserve(N)
        hs.append_events(*s_stream)
        on_dev = args.backend == "nccl"   # RCCL moves device tensors; gloo (functional runs on one GPU) gets host-staged rows
        ss = part_mod.StrongSplit(dist, rank, world, device=dev if on_dev else None)
        back = part_mod.HipRangeBackend(hs, dev) if on_dev else part_mod.HostStagedRangeBackend(hs, dev)

        def strong_step():
            hs.rewind()
            ss.divide_rounds(back, N)
            return ss.decide_fame(back)

        for _ in range(max(1, args.warmup)):
            nc_s = strong_step()
        barrier()
        ts0 = time.perf_counter()
        for _ in range(args.steps):
            nc_s = strong_step()
        barrier()
        dts = rep.max_over_ranks(time.perf_counter() - ts0)
        pv, fx, rs = hs.range_stats()
        strong = {"events_per_s": round(N * args.steps / dts, 1), "ms_per_step": round(dts / args.steps * 1e3, 3), "parts": world,
                  "rows_broadcast_bytes_per_step": int(N * npad_of(n) * 4), "provisional_entries": pv, "repaired": fx, "ranges_swept_twice": rs,
                  "new_c_last_step": int(len(nc_s)),
                  "what": "sw_rewind + StrongSplit.divide_rounds (range sweeps, %d async broadcasts of int32 rows, replicated round loop) + "
                          "candidate-partitioned decide_fame (one all-reduce), max over ranks" % world}
        hs.close()
    elif npad_of(n) > 256 and (world > 1 or args.emulate_parts > 1):
        # Beyond 256 members the split is INSIDE the iterations of the round loop (include/swirld_hip.h part 3): the band events and
        # the members of an iteration are dealt to the parts, which store into each other's tables (peer-mapped memory) and meet
        # at the two kernel boundaries.  The parts are contexts of ONE process — rank 0 drives one context per GPU of the node
        # from one host thread each; the other ranks wait at the barrier (world == 1: --emulate-parts contexts on the one GPU, a
        # functional run).
        P = world if world > 1 else args.emulate_parts
        spread = world > 1 and torch.cuda.device_count() >= P
        devs = list(range(P)) if spread else [local_rank] * P
        if rank == 0:
            s_stream = pkg.synth_hashgraph(n, N, args.seed, args.mode, args.p0, args.p1)
            hp = []
            for d in devs:
                h_ = pkg.Hashgraph(n, device=d)
                h_.reserve(N)
                h_.append_events(*s_stream)
                hp.append(h_)
            pkg.Hashgraph.split_link(hp)
            gate = threading.Barrier(P)
            res = [None] * P

            def part_steps(i, k):
                for _ in range(k):
                    hp[i].rewind()
                    hp[i].synchronize()
                    gate.wait()          # (a part's first band kernel stores into the others' tables: nobody divides before everybody has rewound)
                    hp[i].divide_rounds(0, N)
                    res[i] = [int(r) for r in hp[i].decide_fame()]

            def all_parts(k):
                ths = [threading.Thread(target=part_steps, args=(i, k)) for i in range(P)]
                for t_ in ths:
                    t_.start()
                for t_ in ths:
                    t_.join()

            all_parts(max(1, args.warmup))
            torch.cuda.synchronize()
            ts0 = time.perf_counter()
            all_parts(args.steps)
            dts = time.perf_counter() - ts0
            assert all(r == res[0] for r in res) and res[0] == [int(r) for r in new_c], "every part ends with the replicas' new_c"
            strong = {"events_per_s": round(N * args.steps / dts, 1), "ms_per_step": round(dts / args.steps * 1e3, 3), "parts": P,
                      "devices": devs, "one_gpu_per_part": bool(spread), "new_c_last_step": len(res[0]),
                      "round_iterations_all_steps": int(hp[0].counters()["round_iterations"]),
                      "what": "sw_rewind + sw_divide_rounds on %d linked contexts (sw_split_link: band events and members of every iteration dealt "
                              "to the parts, peer stores, event meetings at both kernel boundaries; sweep and elections replicated) + sw_decide_fame, "
                              "driven by rank 0, one host thread per part" % P}
            if not spread:
                strong["note"] = ("functional run: the parts share ONE device, their kernels take turns on it — not a multi-GPU figure; "
                                  "profiles/r06_split_pieces_1024x2M.txt has what one part runs per iteration alone on a GPU")
            for h_ in hp:
                h_.close()
        barrier()
    elif world == 1 and args.emulate_parts > 1 and npad_of(n) <= 256:
        dev = torch.device("cuda", local_rank)
        P = args.emulate_parts
        hp = []
        for _ in range(P):
            h_ = pkg.Hashgraph(n, device=local_rank)
            h_.reserve(N)
            h_.append_events(*stream)
            hp.append(h_)
        backs = [part_mod.HipRangeBackend(h_, dev) for h_ in hp]
        cuts = part_mod.chunk_cuts(0, N, P)
        sweep_ms = []
        for k, h_ in enumerate(hp):      # the range sweeps, one at a time: what ONE rank spends before its rows can travel
            h_.synchronize()
            tq = time.perf_counter()
            h_.cansee_range(cuts[k], cuts[k + 1] - cuts[k])
            h_.range_stats()             # (synchronises the sweep stream)
            sweep_ms.append((time.perf_counter() - tq) * 1e3)
            h_.rewind()
        torch.cuda.synchronize()
        tq = time.perf_counter()
        part_mod.emulate_strong_split(backs, N)
        tables = [h_.decide_fame_partial(p_, P) for p_, h_ in enumerate(hp)]
        fam_m, dec_m = part_mod.merge_fame_tables(tables)
        ncs = [list(h_.commit_fame(fam_m, dec_m)) for h_ in hp]
        torch.cuda.synchronize()
        emu_ms = (time.perf_counter() - tq) * 1e3
        assert all(x == ncs[0] for x in ncs) and list(ncs[0]) == list(new_c)
        strong = {"emulated_on_one_gpu": True, "parts": P, "range_sweep_ms_each": [round(x, 3) for x in sweep_ms],
                  "all_parts_one_after_the_other_ms": round(emu_ms, 3),
                  "rows_moved_bytes": int(N * npad_of(n) * 4 * (P - 1)), "range_stats": [h_.range_stats() for h_ in hp],
                  "note": "functional run: P contexts on ONE device take turns, so the elapsed time is not a multi-GPU figure; "
                          "range_sweep_ms_each is what one rank spends before its rows can travel"}
        for h_ in hp:
            h_.close()

    return strong


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=300_000,
                    help="events of the same stream timed through the CPU oracle (0 = skip)")
    ap.add_argument("--contexts", type=int, default=4, help="max resident replicas of the DAG per GPU")
    ap.add_argument("--mode", type=int, default=0, help="generator mode (0 uniform gossip = the benchmark; 1 cliques, 2 slow members, 3 stale other-parents: robustness runs)")
    ap.add_argument("--p0", type=float, default=0.0)
    ap.add_argument("--p1", type=float, default=0.0)
    ap.add_argument("--e2e-steps", type=int, default=3, help="end-to-end passes (host arrays in, results on host); 0 = skip")
    ap.add_argument("--split", choices=["replicas", "strong"], default="replicas",
                    help="which multi-GPU number is `value`: independent replicas (default) or ONE hashgraph over the GPUs")
    ap.add_argument("--strong-timeout", type=int, default=150, help="seconds the one-hashgraph split (world > 1) may take before the line is printed without it (0 = no watchdog)")
    ap.add_argument("--emulate-parts", type=int, default=0,
                    help="1 GPU only: also run the one-hashgraph split with this many contexts on the one device (no parallelism: "
                         "a functional run that reports the per-range sweep time and the rows moved)")
    ap.add_argument("--concurrent", type=int, default=2, help="also time this many contexts dividing at once on the one GPU (0 / 1 = skip)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo with --one-device: a functional "
                                                     "run of the multi-rank code on a box with one GPU)")
    ap.add_argument("--one-device", action="store_true", help="test hook: every rank uses cuda:0 (needs --backend gloo: RCCL refuses two ranks on one device)")
    ap.add_argument("--reference-path", default="/root/reference", help="source tree of the Python reference (timed in-run when present)")
    ap.add_argument("--reference-events", type=int, default=8000, help="prefix of the stream timed through the Python reference (~20 s at 256 members)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides `value`: end to end, find_order, roofline, CPU baseline, concurrent contexts, "
                         "the one-hashgraph split (a plain run leaves those fields null)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (new_c, rounds, witnesses, famous, sampled can_see rows) to DIR/<name>.npy")
    args = ap.parse_args()

    import torch
    rep_mod = importlib.import_module("py-swirld_amd.replicas")
    rank, local_rank, world = rep_mod.dist_env()
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback)")
    if args.one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    # N > 1: independent replicas, one per GPU; the collectives of `value` are the barrier and the max-over-ranks time
    rep = rep_mod.Replicas(backend=args.backend, device=torch.device("cuda", local_rank) if args.backend == "nccl" else None)

    pkg = importlib.import_module("py-swirld_amd")
    n, N = args.members, args.events
    stream = pkg.synth_hashgraph(n, N, rep_mod.replica_seed(args.seed, rank), args.mode, args.p0, args.p1)  # host, untimed
    n_ctx = max(1, min(args.contexts, args.steps + args.warmup))
    ctxs = []
    t_ing0 = time.perf_counter()
    for _ in range(n_ctx):
        h = pkg.Hashgraph(n, device=local_rank)
        h.reserve(N)
        h.append_events(*stream)  # ingest (Node.add_event): outside the timed region of `value`
        ctxs.append(h)
    ingest_s = (time.perf_counter() - t_ing0) / n_ctx
    for h in ctxs:  # set-up: every resident context builds its launch graphs once
        h.divide_rounds(0, N)
        h.decide_fame()

    def one_step(i):
        h = ctxs[i % n_ctx]
        h.rewind()  # ALWAYS inside the timed bracket: every step starts from "events ingested, nothing divided"
        h.divide_rounds(0, N)
        return h.decide_fame()

    def barrier():
        rep.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        one_step(i)
    last = {}

    def timed_step(i):
        last["new_c"] = one_step(args.warmup + i)

    # EXACTLY `steps` steps between barrier + device synchronisation on both sides, the MAX over ranks (replicas.Replicas.timed)
    dt = rep.timed(timed_step, args.steps, sync=torch.cuda.synchronize)
    new_c = last["new_c"]
    ms_per_step = dt / args.steps * 1e3
    value = rep.aggregate_throughput(N, args.steps, dt)   # events all ranks processed / the slowest rank's time
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ctxs[(args.warmup + args.steps - 1) % n_ctx], new_c, args.seed)


    # ---- two passes at once on ONE GPU (two contexts, two host threads): how much of the chip one latency-bound pass leaves
    # idle.  Reported next to `value`, never as `value`: a node divides ONE hashgraph, and ms_per_step is that pass's latency.
    conc = None
    if args.full and args.concurrent > 1 and n_ctx >= args.concurrent and world == 1:
        per = max(2, args.steps // args.concurrent)

        def worker(j):
            hj = ctxs[j]
            for _ in range(per):
                hj.rewind()
                hj.divide_rounds(0, N)
                hj.decide_fame()

        ths = [threading.Thread(target=worker, args=(j,)) for j in range(args.concurrent)]
        torch.cuda.synchronize()
        tcc = time.perf_counter()
        for t_ in ths:
            t_.start()
        for t_ in ths:
            t_.join()
        torch.cuda.synchronize()
        dcc = time.perf_counter() - tcc
        conc = {"contexts": args.concurrent, "events_per_s": round(args.concurrent * per * N / dcc, 1), "passes_each": per,
                "ms_per_pass_each": round(dcc / per * 1e3, 3),
                "note": "independent hashgraph views dividing at the same time on one GPU (the C calls release the GIL); the metric's "
                        "`value` is ONE pass at a time"}

    # ---- end to end: host SoA in -> round[N], witness table, famous, new_c on the host ----
    e2e = None
    if args.full and args.e2e_steps > 0:
        h = ctxs[-1]

        def e2e_step():
            h.reset()                      # forget the events too (device storage stays allocated)
            h.append_events(*stream)
            h.divide_rounds(0, N)
            nc = h.decide_fame()
            return h.rounds(), h.witnesses(), h.famous(), nc

        e2e_step()  # warm-up
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.e2e_steps):
            r_e2e = e2e_step()
        barrier()
        dt_e2e = rep.max_over_ranks(time.perf_counter() - t1) / args.e2e_steps
        e2e = {"events_per_s": round(world * N / dt_e2e, 1), "ms_per_pass": round(dt_e2e * 1e3, 3),
               "includes": "sw_reset + sw_append_events (93 B/event over PCIe: parents, t, 64-byte signature) + "
                           "sw_divide_rounds + sw_decide_fame + round[N] / witness table / famous read-back"}
        assert len(r_e2e[0]) == N and list(r_e2e[3]) == list(new_c)

    # ---- per-kernel roofline table: one extra profiled pass (plain launches, hipEvent pairs) ----
    roofline, cd, find_order_ms, find_order_first_ms, fo_ms, ordered = None, {}, None, None, [], []
    c1 = ctxs[0].counters()
    if args.full:
        h = ctxs[0]
        h.rewind()
        h.set_profiling(True)
        c0 = h.counters()
        h.divide_rounds(0, N)
        new_c_prof = h.decide_fame()
        tm = h.timings()
        c1 = h.counters()
        tally_name = h.tally_kernel   # the step-3 kernel THIS pass used (the library chooses per call, DESIGN.md §4 "Which tally")
        h.set_profiling(False)
        t_fo = time.perf_counter()
        ordered = h.find_order(new_c_prof)   # N1 (outside the metric): reported for information only
        find_order_first_ms = (time.perf_counter() - t_fo) * 1e3   # first call of the context: allocates its buffers, fetches the chain pool
        fo_ms = []
        for _ in range(5):                     # the same call again on the same context, five times: what a running node pays (the first two after the
                                               # buffers were allocated run ~0.8 ms slower than the ones behind them, every time: all five are in the line)
            h.rewind()
            h.divide_rounds(0, N)
            nc2 = h.decide_fame()
            h.synchronize()
            t_fo = time.perf_counter()
            ordered2 = h.find_order(nc2)
            fo_ms.append((time.perf_counter() - t_fo) * 1e3)
            assert np.array_equal(ordered, ordered2)
        find_order_ms = sorted(fo_ms)[2]       # the median of the five
        cd = {k: c1[k] - c0[k] for k in c1}
        wkey = workload_key(n, N, args.mode, args.p0, args.p1)
        traffic, rocprof_us, traffic_commit, traffic_workload, traffic_stale = load_traffic(wkey)

        def fam(name, launches, total_ms, alg_bytes_total, served_by, note=None):
            launches = max(1, int(launches))
            avg_ms = total_ms / launches
            ach = alg_bytes_total / launches / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            d = {"kernel": name, "launches": launches, "avg_launch_us": round(avg_ms * 1e3, 2),
                 "total_ms": round(total_ms, 3), "alg_bytes_per_launch": int(alg_bytes_total / launches),
                 "achieved_GBps": round(ach, 1), "frac": round(ach / PEAK_GBPS, 5),
                 "hbm_bytes_per_launch_pmc": traffic.get(name), "served_by": served_by}
            rp = rocprof_us.get(name)
            if rp:   # this family's time per pass in rocprofv3's plain kernel trace of this workload (profiles/traffic.json): no event brackets in it
                ru = rp * 1e3 / launches
                d["total_ms_rocprof"] = rp
                d["avg_launch_us_rocprof"] = round(ru, 2)
                d["achieved_GBps_rocprof"] = round(alg_bytes_total / launches / (ru * 1e-6) / 1e9, 1)
                d["frac_rocprof"] = round(d["achieved_GBps_rocprof"] / PEAK_GBPS, 5)
                if traffic.get(name):
                    d["frac_hbm_measured"] = round(traffic[name] / (ru * 1e-6) / 1e9 / PEAK_GBPS, 5)
            if note:
                d["note"] = note
            return d

        npad = ((n + 63) // 64) * 64
        cs_impl = int(os.environ.get("SW_CANSEE_IMPL", "6" if npad <= 256 else "3"))
        cs_name = "k_cansee_flow" if cs_impl >= 6 else "k_cansee_stream"
        cs_note = "12n B per event (2 parent rows read, 1 written); bound by the dependency chain of the DAG (about 3.4 N/n levels)"
        if cs_name == "k_cansee_stream":   # the level sweep: the parents' 8n B per event never leave LDS, only the row is written
            cs_note = ("12n B per event algorithmic (2 parent rows read, 1 written); the parent rows come from per-member LDS rings, so 4n B per event "
                       "cross the HBM interface; latency-bound on %d DAG levels (one LDS round trip + one barrier each)" % cd.get("levels", 0))
        if cd.get("chunk_sweeps", 0) > 0:  # the chunk-parallel sweep ran (k_cansee_chunks: the launch's span includes its gated repair kernels)
            cs_name = "k_cansee_chunks"
            cs_note = ("12n B per event (2 parent rows read, 1 written); %d chunks swept concurrently in %d launches, each from a halo of "
                       "32 npad events: the dependency chain per launch is the chunk's, not the sub-batch's; %d provisional entries, "
                       "%d chunks swept twice" % (cd["chunk_sweeps"], tm["cansee_launches"], cd["chunk_provisional"], cd["chunk_resweeps"]))
        kernels = [
            fam(cs_name, tm["cansee_launches"], tm["cansee_kernel_ms"], 12 * n * (N - n), "hbm", cs_note),
            fam("k_resolve_band", tm["resolve_launches"], tm["resolve_ms"], cd["band_events"] * (4 * n + n // 8), "hbm/L2",
                "4n B read + n/8 B written per band event; the replicated resolve step (latency: ~1 000 instructions and two dependent round trips) is most of its time"),
            fam(tally_name, tm["tally_launches"], tm["tally_ms"], cd["tally_evals"] * (4 * n + n * n // 8 + 8), "L2",
                "one can_see row + n gathered n-bit masks per evaluation (%d evaluations this pass%s); the gathers hit the "
                "L2-resident band table, so the rate is an L2-gather rate, not HBM"
                % (cd["tally_evals"], ": the two-level search evaluates only the slots it probes" if tally_name == "k_tally_tree" else "")),
            fam("k_elections", 1, tm["elections_ms"], cd["majority_evals"] * (n // 8), "L2/LDS"),
        ]
        # the dominant kernel: the largest total among the families whose bytes come from HBM, by rocprofv3's durations where
        # the committed trace of this workload gives them (the hipEvent brackets of the profiled pass add 2-3 us to every launch
        # of the loop kernels: 297 launches of 8 us looked longer than 6 launches of 460 us), else by this run's brackets
        hbm_fams = [k for k in kernels if k["served_by"].startswith("hbm")]
        dom = max(hbm_fams, key=lambda k: k.get("total_ms_rocprof", k["total_ms"]))
        dr_b, df_b = algorithmic_bytes(n, cd, N)
        path_gbps = (dr_b + df_b) / (ms_per_step * 1e-3) / 1e9
        # counter-measured HBM bytes of one pass: per-launch figures of the committed --pmc passes x the launches of THIS run
        # (round loop: iterations that did work; finalize / voter masks: one launch per sub-batch)
        hbm_pmc = None
        if traffic:
            per_pass = {cs_name: tm["cansee_launches"], "k_resolve_band": cd["round_iterations"], tally_name: cd["round_iterations"],
                        "k_elections": 1, "k_voter_masks_bits": tm["cansee_launches"],
                        # (round numbers / sees-masks: written by the band pass of k_resolve_band, then one check + one launch for the listed leftovers per sub-batch)
                        "k_finalize_check": tm["cansee_launches"], "k_finalize_listed": tm["cansee_launches"], "k_finalize_events": 0}
            if all(traffic.get(k) is not None for k in (cs_name, "k_resolve_band", tally_name)):
                hbm_pmc = int(sum(traffic.get(k, 0) * v for k, v in per_pass.items()))
        path_frac = round(path_gbps / PEAK_GBPS, 5)
        frac_note = None
        if path_frac > 1.0:
            frac_note = ("above 1: SURVEY.md §8d's algorithmic bytes count the tally's n^2 / 8 mask gathers per event, which this path serves from L2 "
                         "(the band-mask table is a few MB): what crosses the HBM interface is frac_hbm_measured")
        roofline = {
            # the headline fraction is the WHOLE PATH's: algorithmic bytes of one pass / ms_per_step against the HBM
            # peak — `achieved` / `frac`; what the counters saw crossing the HBM interface is `traffic` (bytes per step) /
            # `frac_hbm_measured`.  The kernel named here is the HBM-served family with the largest total time; its own rate is in
            # `dominant_kernel` and in the table.  A family whose bytes are L2 gathers (the tallies) is never quoted against HBM.
            "bound": "hbm", "kernel": dom["kernel"], "achieved": round(path_gbps, 2), "peak": PEAK_GBPS,
            "unit": "GB/s", "frac": path_frac, "frac_note": frac_note, "traffic": hbm_pmc,
            "scope": "whole pass (sw_rewind + sw_divide_rounds + sw_decide_fame): algorithmic bytes per step / ms_per_step; "
                     "traffic = HBM bytes per step by the counters",
            "dominant_kernel": {k: dom.get(k) for k in ("kernel", "launches", "avg_launch_us", "avg_launch_us_rocprof", "alg_bytes_per_launch",
                                                         "achieved_GBps", "frac", "achieved_GBps_rocprof", "frac_rocprof",
                                                         "hbm_bytes_per_launch_pmc", "frac_hbm_measured", "served_by")},
            "traffic_source": ("profiles/traffic.json[%s] (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, separate passes, commit %s, %s); "
                               "not measured by this run" % (wkey, traffic_commit, traffic_workload)) if traffic else
                              ("none: profiles/traffic.json holds no counter pass of workload %s on this kernel source%s"
                               % (wkey, " (STALE: measured on other kernel source)" if traffic_stale else "")),
            "traffic_stale": bool(traffic_stale),
            "hbm_bytes_per_step_pmc": hbm_pmc,
            "frac_hbm_measured": round(hbm_pmc / (ms_per_step * 1e-3) / 1e9 / PEAK_GBPS, 5) if hbm_pmc else None,
            "hbm_bytes_note": "sum over kernel families of (PMC bytes per launch, profiles/traffic.json) x (launches of this run's profiled pass) "
                              "/ ms_per_step: what actually crosses the HBM interface, against algorithmic bytes in frac",
            "avg_launch_us": dom["avg_launch_us"], "launches": dom["launches"],
            "dominant_by": "largest time per pass among the HBM-served kernel families (rocprofv3's plain kernel trace of this workload where profiles/traffic.json has it, else this run's event brackets)",
            "kernels": kernels,
            "path_algorithmic_GBps": round(path_gbps, 2), "path_frac": path_frac,
            "path_note": "whole-pass algorithmic bytes (SURVEY.md §8d) / ms_per_step: the path is bound by its dependency "
                         "chains (DAG levels, rounds), not by bandwidth",
            "counters": {k: cd[k] for k in ("levels", "round_iterations", "tally_evals", "band_events", "voter_evals",
                                            "majority_evals", "coin_votes", "coin_flips", "far_hops",
                                            "chunk_sweeps", "chunk_provisional", "chunk_repaired", "chunk_resweeps",
                                            "finalize_from_rows") if k in cd},
            "phase_ms": {k: round(v, 3) for k, v in (("can_see_stream_span", tm["can_see_ms"]), ("round_loop_span", tm["rounds_ms"]),
                                                     ("aux_finalize_voter_span", tm["finalize_ms"]), ("fame", tm["fame_ms"]))},
            "phase_note": "profiled pass = plain launches with event pairs (slower than the graph-replayed timed steps); "
                          "can_see and aux spans run on their own streams and overlap the round loop",
        }

    # ---- CPU baseline: the oracle (C port of the reference algorithm), 1 core, bounded sample ----
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and args.cpu_sample > 0:
        from oracle.oracle import Oracle
        M = min(args.cpu_sample, N)
        o = Oracle(n)
        o.append_events(*[a[:M] for a in stream])
        tc0 = time.perf_counter()
        o.divide_rounds(0, M)
        o.decide_fame()
        tc = time.perf_counter() - tc0
        cpu_baseline = {"value": round(M / tc, 1), "unit": "events/s", "cores": 1, "kind": "port",
                        "host_cores": os.cpu_count(),
                        "sample": "first %d events of the same stream through oracle/swirld_oracle.c "
                                  "(sequential C restatement of swirld.py:187-277), %.1f s" % (M, tc),
                        "python_reference_note": "the unmodified pure-Python reference cannot travel to the GPU box; in the "
                                                 "authoring container it runs 204 events/s at 256 members (BASELINE.md §3)"}
        # the reference itself: timed in THIS run when its tree is reachable (north_star: "timed on the same box's host cores
        # in the same run"); the GPU box has no /root/reference, there the committed measurement of the authoring
        # container stands in (profiles/time_reference_here.py: same stream, results compared with the oracle)
        live = time_python_reference(args.reference_path, n, stream, args.reference_events) if args.reference_events > 0 else None
        if live and live.get("same_run"):
            cpu_baseline["reference_python"] = live
        else:
            try:
                with open(os.path.join(ROOT, "profiles", "reference_python_timing.json")) as f:
                    rp = json.load(f)
                cpu_baseline["reference_python"] = {k: rp[k] for k in ("events_per_s", "events", "members", "cores", "cpu", "where",
                                                                       "c_oracle_same_prefix_events_per_s",
                                                                       "reference_equals_oracle_on_this_prefix") if k in rp}
                cpu_baseline["reference_python"]["same_run"] = False
                if live:
                    cpu_baseline["reference_python"]["in_run_attempt"] = live.get("error")
            except (OSError, ValueError):
                pass

    value_replicas, ms_replicas = value, ms_per_step

    def rnd(x, k):
        return None if x is None else round(x, k)

    line_lock, line_done = threading.Lock(), [False]

    def emit(strong):
        """rank 0 prints THE JSON line, once (the watchdog of the split below may be the one that calls this)."""
        with line_lock:
            if line_done[0] or rank != 0:
                line_done[0] = True
                return
            line_done[0] = True
        use_strong = args.split == "strong" and strong is not None and "events_per_s" in strong
        value, ms_per_step = (strong["events_per_s"], strong["ms_per_step"]) if use_strong else (value_replicas, ms_replicas)
        out = {
            "metric": "events/sec through divide_rounds+decide_fame", "value": round(value, 1),
            "unit": "events/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "weak" if world == 1 else ("strong" if use_strong else "weak-replicas"),
            "vs_baseline": None, "dtype": "int32", "data": "synthetic",
            "value_end_to_end": e2e["events_per_s"] if e2e else None,
            "end_to_end": e2e,
            "value_replicas": round(value_replicas, 1), "ms_per_step_replicas": round(ms_replicas, 3),
            "value_concurrent_contexts": conc,
            "value_strong": strong["events_per_s"] if strong and "events_per_s" in strong else None,
            "strong": strong,
            "value_with_order": round(N / ((ms_replicas + find_order_ms) * 1e-3), 1) if world == 1 and find_order_ms is not None else None,
            "find_order_ms": rnd(find_order_ms, 3), "find_order_first_call_ms": rnd(find_order_first_ms, 3),
            "find_order_calls_ms": [round(x, 3) for x in fo_ms],
            "config": {"workload": "%d members, %d events, %s hashgraph, one batch "
                                   "divide_rounds + decide_fame per step" % (
                                       n, N, ["uniform-gossip", "two-clique", "slow-member", "stale-other-parent"][args.mode]),
                       "members": n, "events": N, "seed": args.seed,
                       "timed_region": "`value`: sw_rewind + sw_divide_rounds + sw_decide_fame on a hashgraph already RESIDENT in HBM "
                                       "(device-resident, the metric); `value_end_to_end`: SURVEY.md §8(d) 'Timing' — host SoA arrays in "
                                       "-> round[N], witness table, famous, new_c back on the host (ingest and PCIe included)",
                       "parallelism": ("one hashgraph over %d GPUs: event-range can_see split + RCCL row broadcasts + partitioned decide_fame" % world)
                                      if use_strong else ("replicas x%d (no data-path collective); the one-hashgraph split is `value_strong`" % world),
                       "rounds": c1["rounds"], "ingest_s_untimed": round(ingest_s, 3),
                       "new_c_last_step": int(len(new_c)),
                       "coin_round_votes": cd.get("coin_votes"), "coin_round_votes_from_signature_bit": cd.get("coin_flips"),
                       "generator": {"mode": args.mode, "p0": args.p0, "p1": args.p1},
                       "find_order_ms_untimed": rnd(find_order_ms, 2), "events_ordered": int(len(ordered)) if args.full else None},
            "roofline": roofline, "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)

    # ---- ONE hashgraph over the GPUs (north_star's split): the same stream on every rank.  LAST, and under a
    # watchdog: everything the line needs besides `strong` exists by now, so a collective of the split that never completes
    # (a rank that failed alone, a fabric problem) costs the run `value_strong`, not the line.
    strong = None
    part_mod = importlib.import_module("py-swirld_amd.partition")
    def on_timeout():
        emit({"error": "the one-hashgraph split did not finish within %d s (a collective did not complete); "
                       "the replicas figures above are unaffected" % args.strong_timeout})

    def run_split():
        try:
            return strong_section(args, pkg, part_mod, rep, torch, rank, local_rank, world, n, N, stream, new_c, barrier)
        except Exception as exc:  # noqa: BLE001 — the replicas line is still printed; the failure is part of it
            return {"error": repr(exc)}

    if args.full or args.split == "strong" or args.emulate_parts > 1:
        strong = guarded(run_split, args.strong_timeout if world > 1 else 0, on_timeout, linger_s=1.0 if rank == 0 else 3.0)
    emit(strong)
    rep.close()


if __name__ == "__main__":
    main()
