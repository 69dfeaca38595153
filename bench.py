#!/usr/bin/env python
"""Benchmark of the ConvONet-Opt restoration path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...)

One "step" = one pass of the whole hot path (SOR -> preprocess/subset/init -> encoder -> 501 Adam steps ->
normalise -> all-gather) over one batch of synthetic ModelNet40-test-like input: 2468 clouds x 1024 points per
GPU (BASELINE.json configs[1]; weak scaling: every rank restores its own 2468 clouds of a 2468*N array).
`value` is BASELINE configs[1] taken literally: ONE file at a time, a device synchronisation after every file - no pass
rides on another's tail (round-4 verdict).  The same passes driven as a stream of files (the next file's pre-processing on a
second HIP stream under the optimiser's last round: a directory of .npz files through the CLI) are `extras.streamed`
(`--streamed` makes that the timed mode).  Inputs are resident in HBM when the timed region starts; weights are seeded
random (the trained checkpoint and ModelNet40 are downloads).  Prints ONE JSON line on rank 0.

A plain run does only what the headline needs: set up, W warm-up passes, K timed passes, the line (its `roofline` object
comes from the events of the timed passes).  `--full` adds everything measured beside it, each in runs of its own: the
CPU baseline, `extras` (streamed driving, reference-style GPU baseline, trained-like field, K = 2048, ONet-Opt, ONet-Mesh,
split precision), `f32_equivalent`, and for N > 1 weak scaling the strong-scaling figure.  `--dump-outputs DIR` writes
the restored clouds of the last timed pass as DIR/restored_points.npy (float32; inputs and weights are seeded, so two
builds can be compared output for output).
"""
import argparse
import json
import os
import re
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # the host driver only supports dmabuf IPC (RCCL over xGMI)

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_CLOUDS = 2468          # ModelNet40 test-set size
K_POINTS = 1024
ITERATIONS = 500         # -> 501 Adam steps (opt_defense.py:210)
FLOP_DENSE_PER_CLOUD = 2 * 15488 * 2 * K_POINTS * (ITERATIONS + 1)     # decoder fwd + input-bwd, SURVEY 8d
F32_MFMA_PEAK_TFLOPS = 157.3                                          # MI355X_MICROARCH.md


def synth_clouds(n, seed=1234, start=0):
    """Area-uniform samples of 7 shape families, unit-sphere normalised like ModelNet40 inputs.
    Cloud i (global index start + i) is drawn from its own generator keyed by (seed, index), so a rank can synthesise
    just its shard and the array is the same whatever the world size."""
    air = np.load(os.path.join(ROOT, "tests", "golden", "convonet_golden.npz"))["raw"][0]
    out = np.empty((n, K_POINTS, 3), np.float32)
    rng = None

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def box(ext, m):
        ext = np.asarray(ext, np.float64)
        area = np.array([ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[1]])
        ax = rng.choice(3, m, p=area / area.sum())
        p = rng.uniform(-1, 1, (m, 3)) * ext
        p[np.arange(m), ax] = rng.choice([-1.0, 1.0], m) * ext[ax]
        return p

    for i in range(n):
        rng = np.random.default_rng((seed, start + i))
        kind = (start + i) % 7
        if kind == 0:
            p = unit(rng.standard_normal((K_POINTS, 3)))
        elif kind == 1:
            p = unit(rng.standard_normal((K_POINTS, 3))) * rng.uniform(0.4, 1.0, 3)
        elif kind == 2:
            p = box(rng.uniform(0.3, 1.0, 3), K_POINTS)
        elif kind == 3:
            a, h = rng.uniform(0, 2 * np.pi, K_POINTS), rng.uniform(-1, 1, K_POINTS)
            r = rng.uniform(0.3, 0.8)
            p = np.stack([r * np.cos(a), r * np.sin(a), h], 1)
        elif kind == 4:
            a, b = rng.uniform(0, 2 * np.pi, (2, K_POINTS))
            t = rng.uniform(0.2, 0.4)
            p = np.stack([(1 + t * np.cos(b)) * np.cos(a), (1 + t * np.cos(b)) * np.sin(a), t * np.sin(b)], 1)
        elif kind == 5:
            m = K_POINTS // 2
            p = np.concatenate([box([0.5, 0.5, 0.08], m), box([0.5, 0.08, 0.5], K_POINTS - m) + [0, 0.45, 0.45]])
        else:
            th = rng.uniform(0, 2 * np.pi)
            rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
            p = air @ rot.T
        p = p - p.mean(0)
        out[i] = (p / np.linalg.norm(p, axis=1).max()).astype(np.float32)
    return out


def _renorm(p):
    p = p - p.mean(0)
    return (p / np.linalg.norm(p, axis=1).max()).astype(np.float32)


def knn_attack_like(clouds, seed=1234):
    """BASELINE config #3: every point displaced by U(-0.02, 0.02)^3, 5 % of the points pulled into
    3 tight clusters (sigma 0.01), re-normalised.  Parity-test input, not a bench line."""
    rng = np.random.default_rng(seed + 3)
    out = np.empty_like(clouds)
    for i, c in enumerate(clouds):
        p = c.astype(np.float64) + rng.uniform(-0.02, 0.02, c.shape)
        k = len(p)
        moved = rng.choice(k, k // 20, replace=False)
        centres = p[rng.choice(k, 3, replace=False)]
        p[moved] = centres[rng.integers(0, 3, len(moved))] + rng.normal(0.0, 0.01, (len(moved), 3))
        out[i] = _renorm(p)
    return out


def drop_like(clouds, n_drop=200, seed=1234):
    """BASELINE config #5(i): delete the n_drop points nearest a random anchor (what untargeted_drop_attack.py
    --num_drop=200 emits: [N, K - n_drop, 3])."""
    rng = np.random.default_rng(seed + 5)
    out = np.empty((len(clouds), clouds.shape[1] - n_drop, 3), np.float32)
    for i, c in enumerate(clouds):
        anchor = c[rng.integers(0, len(c))]
        keep = np.sort(np.argsort(((c - anchor) ** 2).sum(1))[n_drop:])
        out[i] = c[keep]
    return out


def subsample_like(clouds, k=256, seed=1234):
    """BASELINE config #5(ii): K = 256 random subsample of every cloud (sparse input -> 1024 restored points)."""
    rng = np.random.default_rng(seed + 6)
    return np.stack([c[np.sort(rng.choice(len(c), k, replace=False))] for c in clouds]).astype(np.float32)


def usable_cpus():
    """CPUs this process may run on: its affinity mask, bounded by OMP_NUM_THREADS where that is set (a shared host's budget
    per job; os.cpu_count() is the whole host's, and threads or workers sized by it only slow each other down)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    env = os.environ.get("OMP_NUM_THREADS", "")
    if env.isdigit() and int(env) > 0:
        n = min(n, int(env))
    return max(1, n)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, points):
    """--dump-outputs: what the timed path returned in its last pass, the restored clouds [clouds, 1024, 3], as d/restored_points.npy
    (float32).  Above 64 MB (weak scaling over many ranks) an evenly spaced fixed subset of the clouds, whose global indices go to
    d/restored_points_cloud_index.npy (float64)."""
    os.makedirs(d, exist_ok=True)
    a = points.detach().cpu().numpy().astype(np.float32, copy=False)
    per_cloud = a[0].nbytes + 8
    if len(a) * per_cloud > DUMP_LIMIT_BYTES:
        idx = np.arange(0, len(a), -(-len(a) // (DUMP_LIMIT_BYTES // per_cloud)))
        a = a[idx]
        np.save(os.path.join(d, "restored_points_cloud_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(d, "restored_points.npy"), np.ascontiguousarray(a))


def host_cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def kernel_source_sha(precision="f32"):
    """Hash of the optimiser kernel's sources (the stamp scripts/summarise_profiles.py puts on roofline_traffic*.json)."""
    import hashlib
    h = hashlib.sha256()
    files = ("optimize.hip", "optimize_kernel.h", "knn_device.h", "ifd_device.h")
    if precision != "f32":
        files += ("optimize_bf.hip", "tile_bf.h", "split_bf16.h")
    for f in files:
        h.update(open(os.path.join(ROOT, "if-defense_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def launch_shapes_of(ev, flop_per_cloud):
    """[(clouds, mean ms, fraction of the f32-MFMA peak)] of the optimiser launches in `ev` ((event, event, clouds) triples), largest first."""
    shapes = {}
    for e0, e1, n_ in ev:
        shapes.setdefault(n_, []).append(e0.elapsed_time(e1))
    return [{"clouds": n_, "ms": round(sum(v) / len(v), 2),
             "frac": round(flop_per_cloud * n_ / (sum(v) / len(v) * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4)}
            for n_, v in sorted(shapes.items(), reverse=True)]


def traffic_from_profiles(precision, clouds_per_file, launches_per_file):
    """HBM-side bytes per average launch from the PMC passes committed under profiles/ (counters cannot be read inside this run):
    quoted only if they were measured on THIS kernel (source hash), this file size and this launch scheme - else None + the reason."""
    name = "roofline_traffic.json" if precision == "f32" else "roofline_traffic_%s.json" % precision
    tf = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(tf) or abs(clouds_per_file - N_CLOUDS) > 0.5:
        return None, None, None
    tj = json.load(open(tf))
    if tj.get("kernel_source_sha") == kernel_source_sha(precision) and tj.get("launches_per_file", 1) == launches_per_file:
        return (tj.get("optimize_kernel_hbm_bytes_per_launch"),
                "profiles/%s (rocprofv3 PMC passes of this kernel, fetch factor %.2f; %g launch(es) per file, bytes per average launch; "
                "FETCH_SIZE counts L2 -> fabric requests: Infinity-Cache hits are inside it)" % (name, tj.get("fetch_factor", 2.0), launches_per_file),
                tj.get("launch_shapes"))
    return None, "profiles/%s is from another build of the kernel or another launch scheme - not quoted" % name, None


def cpu_baseline(clouds, n_sample=16, budget_s=15.0, onet=False, full_run_clouds=0):
    """The CPU oracle (a port of the reference's op sequence: bmm-kNN + topk, autograd, torch.optim.Adam) timed
    on the host cores on a bounded sample, scaled to 501 steps.  Reported next to the GPU number, not a target.
    Threads are capped at 16: with one thread per core of a 256-core host the small ops of this loop run
    ~100x slower (measured: 22 s per step), which would say nothing about the CPU path."""
    from oracle import convonet_oracle as O
    threads = min(usable_cpus(), 16)
    torch.set_num_threads(threads)
    if onet:
        from oracle import onet_oracle as OO
        MO, w, n_in, encode = OO, OO.to_torch(OO.make_random_weights(0)), 300, OO.encode_latent
    else:
        MO, w, n_in, encode = O, O.to_torch(O.make_random_weights(0)), 600, O.encode_inputs
    x = torch.from_numpy(clouds[:n_sample])
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    keep, _ = O.sor_keep_mask(x)
    proc = [O.preprocess_pc(clouds[b][keep[b].numpy()]) for b in range(n_sample)]
    sel = torch.from_numpy(np.stack([p[rng.choice(len(p), n_in, replace=False)] for p in proc]))
    with torch.no_grad():
        planes = encode(w, sel)
    idx = np.stack([rng.integers(0, len(p), K_POINTS) for p in proc])
    init = O.init_points(proc, idx, rng.standard_normal((n_sample, K_POINTS, 3)).astype(np.float32))
    t_pre = time.perf_counter() - t0
    MO.optimize_points(w, init, planes, rep_weight=500.0, iterations=0, normalize=False)      # warm-up step
    t0 = time.perf_counter()
    MO.optimize_points(w, init, planes, rep_weight=500.0, iterations=1, normalize=False)      # 2-step probe
    probe = (time.perf_counter() - t0) / 2
    n_steps = int(max(3, min(50, budget_s / max(probe, 1e-3))))
    t0 = time.perf_counter()
    MO.optimize_points(w, init, planes, rep_weight=500.0, iterations=n_steps - 1, normalize=True)
    t_opt = time.perf_counter() - t0
    per_cloud = (t_pre + t_opt / n_steps * (ITERATIONS + 1)) / n_sample
    out = {"value": round(1.0 / per_cloud, 4), "unit": "clouds/s", "cores": threads, "kind": "port",
           "host_cpu": host_cpu_model(), "host_cores": os.cpu_count(),
           "sample": "%d clouds: SOR+preprocess+encoder once (%.2f s) + %d of %d Adam steps (%.2f s), scaled to %d steps"
                     % (n_sample, t_pre, n_steps, ITERATIONS + 1, t_opt, ITERATIONS + 1)}
    if full_run_clouds and probe * (ITERATIONS + 1) * full_run_clouds / n_sample < 60.0:
        # one complete 501-step run, nothing scaled (a small batch: the per-cloud time is not the 16-cloud one)
        t0 = time.perf_counter()
        MO.optimize_points(w, init[:full_run_clouds], {k: v[:full_run_clouds] for k, v in planes.items()} if isinstance(planes, dict)
                           else planes[:full_run_clouds], rep_weight=500.0, iterations=ITERATIONS, normalize=True)
        t_full = time.perf_counter() - t0
        out["full_run"] = {"clouds": full_run_clouds, "adam_steps": ITERATIONS + 1, "seconds": round(t_full, 2),
                           "clouds_per_s": round(full_run_clouds / (t_full + t_pre * full_run_clouds / n_sample), 4)}
    return out


def _cpu_worker(job):
    """One worker of the host-saturating CPU figure: the oracle's optimiser loop on its own clouds, `threads` intra-op threads."""
    seed, n, steps, threads = job
    import torch as T
    T.set_num_threads(threads)
    from oracle import convonet_oracle as O
    w = O.to_torch(O.make_random_weights(0))
    g = T.Generator().manual_seed(seed)
    v = T.randn(n, K_POINTS, 3, generator=g)
    init = 0.4 * v / v.norm(dim=-1, keepdim=True) + 0.01 * T.randn(n, K_POINTS, 3, generator=g)
    planes = {k: 0.5 * T.randn(n, 32, 64, 64, generator=g) for k in ("xz", "xy", "yz")}
    O.optimize_points(w, init, planes, rep_weight=500.0, iterations=0, normalize=False)      # warm-up step
    t0 = time.perf_counter()
    O.optimize_points(w, init, planes, rep_weight=500.0, iterations=steps - 1, normalize=False)
    return (time.perf_counter() - t0) / steps


def _cpu_worker_cold(job):
    """(no warm-up step: one step of 192 clouds at one thread per core takes half a minute - start-up costs vanish in it)"""
    seed, n, steps, threads = job
    torch.set_num_threads(threads)
    from oracle import convonet_oracle as O
    w = O.to_torch(O.make_random_weights(0))
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, K_POINTS, 3, generator=g)
    init = 0.4 * v / v.norm(dim=-1, keepdim=True) + 0.01 * torch.randn(n, K_POINTS, 3, generator=g)
    planes = {k: 0.5 * torch.randn(n, 32, 64, 64, generator=g) for k in ("xz", "xy", "yz")}
    t0 = time.perf_counter()
    O.optimize_points(w, init, planes, rep_weight=500.0, iterations=steps - 1, normalize=False)
    return (time.perf_counter() - t0) / steps


def cpu_baseline_pick(base):
    """ONE `cpu_baseline.value` (round-5 verdict): every CPU the run may use - usable_cpus() // 16 oracle processes of 16 threads side by side, the
    sampling in which the reference's loop uses the box best - with the once-per-cloud pre-processing of the single-process sample
    added; the other samplings (one 16-thread process; 4 clouds unscaled; one B = 192 batch on all threads) stay beside it."""
    sat = base.get("host_saturating", {}).get("workers_x16_threads", {})
    if "value" not in sat:
        base["definition"] = "one 16-thread oracle process (the host-saturating sampling failed: %s)" % sat.get("error", "?")
        return base
    single = {k: base[k] for k in ("value", "cores", "sample") if k in base}
    try:
        m = re.search(r"once \(([0-9.]+) s\)", base["sample"])
        t_pre_per_cloud = float(m.group(1)) / 16.0
    except Exception:      # noqa: BLE001
        t_pre_per_cloud = 0.0
    v = 1.0 / (1.0 / sat["value"] * 1.0 + t_pre_per_cloud / max(1, sat.get("workers", 1)))
    base["other_samplings"] = {"one_process_16_threads": single, "full_run_4_clouds": base.pop("full_run", None),
                               "batch192_all_threads": base["host_saturating"].get("batch192_all_threads")}
    base.pop("host_saturating", None)
    base.update({"value": round(v, 4), "cores": sat["cores"], "sample": sat["sample"] + "; + SOR / preprocess / encoder once per cloud from the "
                 "one-process sample", "definition": "THE cpu_baseline: every CPU the run may use, %d oracle processes x 16 threads (other_samplings: "
                 "smaller or differently batched samples of the same loop - they differ by up to 30 %% and are not the baseline)" % sat.get("workers", 0)})
    return base


def cpu_baseline_saturating(base, budget_s=20.0):
    """Two host-SATURATING figures next to the 16-thread one (round-4 verdict): (i) floor(cores / 16) concurrent 16-thread workers on
    disjoint 16-cloud batches, (ii) the reference's own batch of 192 clouds in ONE process at one thread per core (BASELINE.md
    section 3's setting).  Optimiser loop only (96 % of the path's CPU time), a few steps each, scaled to 501; bounded.  cores =
    usable_cpus(), the CPUs this run may use; at most 15 workers, so that with this process no more than 16 hold the GPU open."""
    import multiprocessing as mp
    cores = usable_cpus()
    out = {}
    per_step_16 = None
    try:
        m = re.search(r"(\d+) of \d+ Adam steps \(([0-9.]+) s\)", base["sample"])
        per_step_16 = float(m.group(2)) / int(m.group(1))
    except Exception:      # noqa: BLE001
        pass
    try:
        workers = max(1, min(15, cores // 16))
        steps = 3 if per_step_16 is None else int(max(2, min(10, budget_s / (3.0 * per_step_16))))
        with mp.get_context("spawn").Pool(workers) as pool:
            t0 = time.perf_counter()
            per = pool.map(_cpu_worker, [(100 + i, 16, steps, 16) for i in range(workers)])
            wall = time.perf_counter() - t0
        slowest = max(per)
        out["workers_x16_threads"] = {
            "value": round(workers * 16 / (slowest * (ITERATIONS + 1)), 4), "unit": "clouds/s", "cores": workers * 16, "workers": workers,
            "sample": "%d concurrent workers x 16 threads x 16 clouds, %d Adam steps each (slowest worker %.2f s per step, pool wall "
                      "%.1f s incl. start-up), optimiser loop only, scaled to %d steps" % (workers, steps, slowest, wall, ITERATIONS + 1)}
    except Exception as e:      # noqa: BLE001
        out["workers_x16_threads"] = {"error": str(e)[:200]}
    try:
        t0 = time.perf_counter()
        per = _cpu_worker_cold((7, 192, 1, cores))
        out["batch192_all_threads"] = {
            "value": round(192 / (per * (ITERATIONS + 1)), 4), "unit": "clouds/s", "cores": cores,
            "sample": "ONE process, torch.set_num_threads(%d), the reference's batch of 192 clouds: 1 timed Adam step (%.2f s), "
                      "optimiser loop only, scaled to %d steps (%.1f s in all)" % (cores, per, ITERATIONS + 1, time.perf_counter() - t0)}
    except Exception as e:      # noqa: BLE001
        out["batch192_all_threads"] = {"error": str(e)[:200]}
    return out


def timed_files(r, x, args, lo, total, ev, n_files, warm=1):
    """`n_files` files one at a time (a device synchronisation after each, like the headline), after `warm` untimed ones:
    (seconds per file, the optimiser launches' events of the timed files)."""
    import ifdefense_amd as I
    for _ in I.defend_stream(r, [x] * warm, args, bases=[lo] * warm, totals=[total] * warm, overlap=False):
        torch.cuda.synchronize()
    ev.clear()
    t0 = time.perf_counter()
    for _ in I.defend_stream(r, [x] * n_files, args, bases=[lo] * n_files, totals=[total] * n_files, overlap=False):
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_files, list(ev)


def f32_equivalent_block(r, x, args, lo, total, ev, n_files=4):
    """The SAME workload with the decoder's dense layers on the bf16 matrix core, every operand split exactly into three bf16 pieces,
    six piece products, f32 accumulation (ifd_opt_params.precision = 1, "bf16x6"; csrc/tile_bf.h): f32-EQUIVALENT arithmetic - its
    error against float64 equals the f32 MFMA chain's, and the whole GPU parity matrix runs in this mode at the f32 bars
    (tests/conftest.py `both_precisions`).  Reported beside the headline, never in its place (round-5 verdict, item 1)."""
    import dataclasses
    a6 = dataclasses.replace(args, precision="bf16x6")
    dt, evs = timed_files(r, x, a6, lo, total, ev, n_files)
    ms = [e0.elapsed_time(e1) for e0, e1, _ in evs]
    clouds = [n for _, _, n in evs]
    avg_ms, avg_clouds = sum(ms) / len(ms), sum(clouds) / len(clouds)
    achieved = FLOP_DENSE_PER_CLOUD * avg_clouds / (avg_ms * 1e-3) / 1e12
    launches_per_file = len(ms) / float(n_files)
    traffic, src, shapes_t = traffic_from_profiles("bf16x6", sum(clouds) / float(n_files), launches_per_file)
    return {"mode": "bf16x6", "value": round(total / dt, 2), "unit": "clouds/s", "files_timed": n_files, "ms_per_file": round(dt * 1e3, 2),
            "dtype": "bf16x6 (f32-equivalent: three exact bf16 pieces per operand, six products on v_mfma_f32_16x16x32_bf16, f32 accumulation)",
            "roofline": {"bound": "mfma", "kernel": "ifd::optimize_kernel<8, S, 1>", "achieved": round(achieved, 2), "peak": F32_MFMA_PEAK_TFLOPS,
                         "unit": "TFLOP/s (f32-equivalent: algorithmic decoder FLOPs; the matrix core executes 6x as many bf16 FLOPs, its dense "
                                 "bf16 peak is ~2500)", "frac": round(achieved / F32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                         "traffic_source": src, "traffic_launch_shapes": shapes_t, "launch_ms": round(avg_ms, 2), "clouds_per_launch": avg_clouds,
                         "launches_per_file": launches_per_file, "launch_shapes": launch_shapes_of(evs, FLOP_DENSE_PER_CLOUD)},
            "parity": "tests/test_gpu_parity.py (the `both_precisions` tests: configs #3 / #5 attribution, 16 clouds x 20 steps, P3 501 steps, "
                      "full size 2468 x 501 with bitwise re-runs, point-count sweep, large clouds, trained-like to t = 500, ONet config #1) and "
                      "tests/test_gpu_split_precision.py - all at the f32 path's own bars",
            "what": "the headline workload, driver and timing, only ifd_opt_params.precision differs; opt-in (--precision bf16x6), not the metric"}


def split_precision_extras(r, x, args, lo, total, ev):
    """SURVEY 8f row N4, the REDUCED mode: bf16x3 = two bf16 pieces per operand, three products (2^-17 per product) - characterised in
    tests/test_gpu_split_precision.py, never the headline.  (bf16x6, the f32-equivalent mode, has its own block: `f32_equivalent`.)"""
    import dataclasses
    out = {}
    try:
        dt, evs = timed_files(r, x, dataclasses.replace(args, precision="bf16x3"), lo, total, ev, 2)
        ms = sum(e0.elapsed_time(e1) for e0, e1, _ in evs) / 2.0          # per FILE: the sum of its launches (partial round + whole rounds)
        out["bf16x3"] = {"value": round(total / dt, 1), "unit": "clouds/s", "ms_per_file": round(dt * 1e3, 1), "optimiser_launch_ms": round(ms, 1),
                         "f32_equivalent_tflops": round(FLOP_DENSE_PER_CLOUD * total / (ms * 1e-3) / 1e12, 1),
                         "precision": "REDUCED (two pieces, three products: 2^-17 per product)"}
    except Exception as e:      # noqa: BLE001
        out["bf16x3"] = {"error": str(e)[:200]}
    out["what"] = ("opt-in REDUCED-precision arithmetic of the decoder's 32 x 32 layers, never the headline: one 2468-cloud file at a time, mean "
                   "of 2; optimiser_launch_ms = the file's optimiser launches together")
    return out


def trained_like_full(dev, n=N_CLOUDS, n_files=2):
    """Round-5 verdict, item 6: a headline-SHAPED run on the realistic field - 2468 clouds, all seven bench families interleaved (one in
    seven an airplane the checkpoint never saw), the trained-like checkpoint (tests/golden/trained_like_f16.npz), the WHOLE pipeline one
    file at a time - with the launch shapes and the neighbour-list counters of the last file."""
    import ifdefense_amd as I
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_like_f16.npz"))
    r = I.Restorer(I.weights.pack_state_dict({k: z[k].astype(np.float32) for k in z.files}), device=dev)
    try:
        x = torch.from_numpy(synth_clouds(n)).to(dev)
        args = I.DefenseArgs(iterations=ITERATIONS, seed=1234)
        ev = []
        orig = r.optimize_points

        def timed(*p, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = orig(*p, **k)
            e1.record()
            ev.append((e0, e1, o.shape[0]))
            return o

        r.optimize_points = timed
        dt, evs = timed_files(r, x, args, 0, n, ev, n_files)
        c = r.counters()                                           # of the last launch: the file's whole rounds
        last_n = evs[-1][2]
        ms = [e0.elapsed_time(e1) for e0, e1, _ in evs]
        clouds = [k for _, _, k in evs]
        achieved = FLOP_DENSE_PER_CLOUD * (sum(clouds) / len(clouds)) / (sum(ms) / len(ms) * 1e-3) / 1e12
        return {"value": round(n / dt, 1), "unit": "clouds/s (whole path, one file at a time)", "ms_per_file": round(dt * 1e3, 1),
                "roofline_frac": round(achieved / F32_MFMA_PEAK_TFLOPS, 4), "launch_shapes": launch_shapes_of(evs, FLOP_DENSE_PER_CLOUD),
                "list_rebuilds_per_cloud": round(c["knn_rebuilds"] / 8.0 / last_n, 2),
                "ring_use_fraction": round(c["knn_ring_evals"] / (8.0 * last_n * (ITERATIONS + 1)), 3),
                "exact_query_fraction": round(c["knn_exact_evals"] / (8.0 * last_n * (ITERATIONS + 1)), 4),
                "what": "%d clouds of all SEVEN bench families, trained-like checkpoint, SOR + preprocess + encode + init + 501 Adam steps + "
                        "normalise, %d files timed one at a time (f32); counters of the last file's whole-rounds launch" % (n, n_files)}
    finally:
        r.close()


def extras(dev):
    """Bounded side measurements carried in the N = 1 --full line (a few seconds each; none of them is the headline):
    the reference's op sequence run unfused by PyTorch-ROCm on the same GPU, and the two ONet rows of SURVEY 8f."""
    import ifdefense_amd as I
    out = {}
    try:      # reference-style GPU baseline: the oracle's ops (bmm kNN + topk, autograd, torch.optim.Adam), one kernel per op
        from oracle import convonet_oracle as O
        n, steps = 64, 20
        w = {k: v.to(dev) for k, v in O.to_torch(O.make_random_weights(0)).items()}
        clouds = synth_clouds(n)
        t0 = time.perf_counter()
        keep, _ = O.sor_keep_mask(torch.from_numpy(clouds).to(dev))
        keep = keep.cpu().numpy().astype(bool)
        procs = [O.preprocess_pc(clouds[b][keep[b]]) for b in range(n)]
        g = torch.Generator().manual_seed(0)
        sel = torch.stack([torch.from_numpy(p[torch.randperm(len(p), generator=g)[:600].numpy()]) for p in procs]).to(dev)
        init = torch.stack([torch.from_numpy(p[torch.randint(len(p), (K_POINTS,), generator=g).numpy()]) for p in procs])
        init = (init + 0.01 * torch.randn(init.shape, generator=g)).clamp(-0.45, 0.45).to(dev)
        with torch.no_grad():
            planes = O.encode_inputs(w, sel)
        torch.cuda.synchronize()
        t_pre = time.perf_counter() - t0
        O.optimize_points(w, init[:2], {k: v[:2] for k, v in planes.items()}, iterations=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        O.optimize_points(w, init, planes, rep_weight=500.0, iterations=steps - 1)
        torch.cuda.synchronize()
        t_opt = time.perf_counter() - t0
        out["reference_style_gpu"] = {"value": round(n / (t_pre + t_opt * (ITERATIONS + 1.0) / steps), 2), "unit": "clouds/s",
                                      "what": "the reference's op sequence (oracle) run unfused by PyTorch-ROCm on this GPU: %d clouds, "
                                              "%d of %d Adam steps timed, scaled" % (n, steps, ITERATIONS + 1)}
    except Exception as e:      # noqa: BLE001  (a side measurement must never take the headline line down)
        out["reference_style_gpu"] = {"error": str(e)[:200]}
    try:      # the converged-surface regime: the optimiser on a TRAINED-LIKE field (tests/golden/train_trained_like.py)
        z = np.load(os.path.join(ROOT, "tests", "golden", "trained_like_f16.npz"))
        r = I.Restorer(I.weights.pack_state_dict({k: z[k].astype(np.float32) for k in z.files}), device=dev)
        n = 512                                                     # two whole rounds of one cloud per CU
        pool = synth_clouds(602)                                    # the six shape families the checkpoint was trained on
        x = torch.from_numpy(pool[np.arange(602) % 7 != 6][:n]).to(dev)      # (family 6, the airplane, has no analytic occupancy)
        prep = r.prepare(x, r.sor(x), seed=1234)
        planes = r.encode_inputs(prep["sel"], prep["t_per_cloud"])
        lb = torch.full((n,), 192, dtype=torch.int32, device=dev)
        r.optimize_points(prep["init"][:8], planes[:8], rep_weight=500.0, steps=2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pts = r.optimize_points(prep["init"], planes, rep_weight=500.0, iterations=ITERATIONS, loss_batch=lb, normalize=False)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        c = r.counters()
        p0 = torch.sigmoid(r.decode(prep["init"], planes))
        p1 = torch.sigmoid(r.decode(pts, planes))
        out["trained_like"] = {
            "value": round(n / (ms * 1e-3), 1), "unit": "clouds/s (optimiser launch only)",
            "roofline_frac": round(FLOP_DENSE_PER_CLOUD * n / (ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
            "list_rebuilds_per_cloud": round(c["knn_rebuilds"] / 8.0 / n, 2),
            "ring_use_fraction": round(c["knn_ring_evals"] / (8.0 * n * (ITERATIONS + 1)), 3),
            "exact_query_fraction": round(c["knn_exact_evals"] / (8.0 * n * (ITERATIONS + 1)), 4),
            "occupancy_prob_abs_dev_from_threshold": {"init": round(float((p0 - 0.2).abs().mean()), 4),
                                                      "restored": round(float((p1 - 0.2).abs().mean()), 4)},
            "what": "ifd_optimize on %d bench clouds of the six trained shape families with the trained-like checkpoint "
                    "(tests/golden/trained_like_f16.npz: the reference model trained on analytic occupancy of those families; "
                    "a field with a surface at the iso-value 0.2), 501 Adam steps, one workgroup per cloud" % n}
        # the family the checkpoint never saw (the airplane): an untrained field under trained weights - the slowest clouds
        xa = torch.from_numpy(pool[np.arange(602) % 7 == 6][:64]).to(dev)
        pa = r.prepare(xa, r.sor(xa), seed=1234)
        pla = r.encode_inputs(pa["sel"], pa["t_per_cloud"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.optimize_points(pa["init"], pla, rep_weight=500.0, iterations=ITERATIONS, loss_batch=lb[:64], normalize=False, split=1)
        e1.record()
        torch.cuda.synchronize()
        ca = r.counters()
        out["trained_like"]["unseen_family"] = {
            "ms_per_round": round(e0.elapsed_time(e1), 1), "vs_trained_families": round(e0.elapsed_time(e1) / (ms / 2.0), 3),
            "list_rebuilds_per_cloud": round(ca["knn_rebuilds"] / 8.0 / 64, 2),
            "what": "64 airplane clouds (one partial round, one workgroup per cloud) on the same checkpoint"}
        # all seven families in ONE launch (what a real file looks like: the slowest clouds of a round set its length)
        xm = torch.from_numpy(pool[:n]).to(dev)
        pm = r.prepare(xm, r.sor(xm), seed=1234)
        plm = r.encode_inputs(pm["sel"], pm["t_per_cloud"])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.optimize_points(pm["init"], plm, rep_weight=500.0, iterations=ITERATIONS, loss_batch=lb, normalize=False)
        e1.record()
        torch.cuda.synchronize()
        cm = r.counters()
        msm = e0.elapsed_time(e1)
        out["trained_like_mixed"] = {
            "value": round(n / (msm * 1e-3), 1), "unit": "clouds/s (optimiser launch only)",
            "roofline_frac": round(FLOP_DENSE_PER_CLOUD * n / (msm * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
            "list_rebuilds_per_cloud": round(cm["knn_rebuilds"] / 8.0 / n, 2),
            "what": "the same launch with all SEVEN bench families interleaved (%d clouds, one in seven an airplane the "
                    "checkpoint never saw): two whole rounds whose length the slowest clouds set" % n}
        r.close()
    except Exception as e:      # noqa: BLE001
        out["trained_like"] = {"error": str(e)[:200]}
    try:      # clouds of more than 1024 optimised points (--sample_npoint 2048): the two-launch-per-step path against the persistent kernel
        w = I.weights.pack_state_dict(I.weights.random_state_dict(0))
        r = I.Restorer(w, device=dev)
        x = torch.from_numpy(synth_clouds(256)).to(dev)
        per = {}
        first101 = {}
        for k_opt, steps in ((1024, 101), (2048, 101), (1024, ITERATIONS + 1), (2048, ITERATIONS + 1)):
            prep = r.prepare(x, r.sor(x), n_sel=600, n_opt=k_opt, seed=1234)
            planes = r.encode_inputs(prep["sel"], prep["t_per_cloud"])
            r.optimize_points(prep["init"][:8], planes[:8], rep_weight=500.0, steps=2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.optimize_points(prep["init"], planes, rep_weight=500.0, steps=steps)
            torch.cuda.synchronize()
            per[k_opt] = (time.perf_counter() - t0) / (256.0 * k_opt * steps)
            if steps == 101:
                first101[k_opt] = per[k_opt]
            ck = r.counters()
        # ... and on a file-sized batch (2304 clouds = nine rounds of the persistent kernel; pipeline.py hands a whole file to one call):
        # with more clouds than CUs a list-step launch costs the AVERAGE cloud, not the slowest of 256
        xf = torch.from_numpy(synth_clouds(9 * 256)).to(dev)
        perf = {}
        for k_opt in (1024, 2048):
            prep = r.prepare(xf, r.sor(xf), n_sel=600, n_opt=k_opt, seed=1234)
            planes = r.encode_inputs(prep["sel"], prep["t_per_cloud"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.optimize_points(prep["init"], planes, rep_weight=500.0, steps=ITERATIONS + 1)
            torch.cuda.synchronize()
            perf[k_opt] = (time.perf_counter() - t0) / (9 * 256.0 * k_opt * (ITERATIONS + 1))
            del prep, planes
        out["k2048"] = {"value": round(1.0 / (per[2048] * 2048 * (ITERATIONS + 1)), 2), "unit": "clouds/s (2048 optimised points each, optimiser only)",
                        "per_point_cost_vs_1024": round(per[2048] / per[1024], 2),
                        "per_point_cost_vs_1024_first_101_steps": round(first101[2048] / first101[1024], 2),
                        "per_point_cost_vs_1024_file_sized_batch": round(perf[2048] / perf[1024], 2),
                        "value_file_sized_batch": round(1.0 / (perf[2048] * 2048 * (ITERATIONS + 1)), 2),
                        "whole_cloud_list_builds_per_cloud": round(ck["knn_rebuilds"] / 256.0, 2),
                        "exact_query_fraction": round(ck["knn_exact_evals"] / (256.0 * 2048 * (ITERATIONS + 1)), 5),
                        "what": "ifd_optimize on 256 clouds x 2048 points (two launches per Adam step: the persistent kernel's decoder tile, then certified "
                                "neighbour lists + repulsion + Adam: DESIGN section 4.6), all 501 steps, nothing scaled; per_point_cost_vs_1024 = time per "
                                "point and step over the persistent kernel's on 256 clouds x 1024 x 501 steps (and over the first 101 steps of both, where "
                                "the persistent kernel still rebuilds its lists often); _file_sized_batch: the same ratio on 2304 clouds in one call "
                                "(a launch ends with its slowest cloud; batches go as up to four stream groups that fill each other's idle CUs, "
                                "and with more clouds than CUs a launch costs nearer its average cloud)"}
        r.close()
    except Exception as e:      # noqa: BLE001
        out["k2048"] = {"error": str(e)[:200]}
    try:      # ONet-Opt decoder variant: 256 clouds x 51 steps, scaled to 501
        r = I.OnetRestorer(I.weights.pack_state_dict(I.weights.onet_random_state_dict(0), "onet"), device=dev)
        x = torch.from_numpy(synth_clouds(256)).to(dev)
        prep = r.prepare(x, r.sor(x), n_sel=300, seed=1234)
        c = r.encode_inputs(prep["sel"], prep["t_per_cloud"])
        r.optimize_points(prep["init"][:8], c[:8], rep_weight=500.0, steps=2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.optimize_points(prep["init"], c, rep_weight=500.0, steps=51)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        flop = 256 * K_POINTS * 51 * 2 * 2 * (10 * 256 * 256 + 4 * 256)
        out["onet_opt"] = {"value": round(256 / (dt * (ITERATIONS + 1) / 51), 2), "unit": "clouds/s",
                           "roofline_frac": round(flop / dt / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
                           "what": "ifd_onet_optimize, 256 clouds x 51 of 501 Adam steps, scaled (optimiser only)"}
        sp = {}
        for mode in ("bf16x6", "bf16x3"):     # the opt-in split-precision passes of the same launch (onet_kernel.h onet_pass_bf)
            r.optimize_points(prep["init"][:8], c[:8], rep_weight=500.0, steps=2, precision=mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.optimize_points(prep["init"], c, rep_weight=500.0, steps=51, precision=mode)
            torch.cuda.synchronize()
            dts = time.perf_counter() - t0
            sp[mode] = {"value": round(256 / (dts * (ITERATIONS + 1) / 51), 2), "unit": "clouds/s",
                        "f32_equivalent_tflops": round(flop / dts / 1e12, 1),
                        "precision": "f32-equivalent" if mode == "bf16x6" else "REDUCED (2^-17 relative per product)"}
        out["onet_opt"]["split_precision"] = sp
        # ONet-Mesh: MISE grid + marching cubes + surface samples, threshold at the field's median
        gq = torch.Generator().manual_seed(9)
        med = float(r.decode((torch.rand(8, 4096, 3, generator=gq) - 0.5) * 1.1, c[:8]).median())
        thr = 1.0 / (1.0 + np.exp(-med))
        r.mesh_sample(c[:4], threshold=thr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.mesh_sample(c[:64], threshold=thr)
        torch.cuda.synchronize()
        dtm = time.perf_counter() - t0
        km = r.counters()
        flop_m = km["mesh_points"] * 2 * (10 * 256 * 256 + 4 * 256)        # decoder forward per evaluated grid point
        out["onet_mesh"] = {"value": round(64 / dtm, 1), "unit": "clouds/s",
                            "grid_points_per_cloud": int(km["mesh_points"] / 64), "mise_rounds": int(km["mesh_rounds"]),
                            "roofline_frac": round(flop_m / dtm / 1e12 / F32_MFMA_PEAK_TFLOPS, 4),
                            "what": "ifd_onet_mesh_sample, 64 clouds, 32 -> 128 MISE grid, iso-surface at the field's median; "
                                    "roofline_frac = decoder FLOPs of the evaluated grid points / WHOLE-path time / f32-MFMA peak "
                                    "(onet_grid_eval_kernel alone: profiles/r05_onet_mesh_kernel_stats.txt)"}
        spm = {}
        for mode in ("bf16x6", "bf16x3"):     # ifd_mesh_params.precision: the grid evaluation on the split-precision passes (opt-in)
            r.mesh_sample(c[:4], threshold=thr, precision=mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r.mesh_sample(c[:64], threshold=thr, precision=mode)
            torch.cuda.synchronize()
            spm[mode] = {"value": round(64 / (time.perf_counter() - t0), 1), "unit": "clouds/s",
                         "precision": "f32-equivalent" if mode == "bf16x6" else "REDUCED (2^-17 relative per product)"}
        out["onet_mesh"]["split_precision"] = spm
        r.close()
    except Exception as e:      # noqa: BLE001
        out["onet"] = {"error": str(e)[:200]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)      # ~1 s per step; the first timed pass has nothing to hide its
    ap.add_argument("--warmup", type=int, default=2)      # pre-processing under, so short runs read ~1.5 % low
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline, in runs of its own: CPU baseline, extras, f32_equivalent, and "
                         "the strong-scaling figure of an N > 1 weak-scaling run (--no-cpu-baseline / --no-extras drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the restored clouds of the last timed pass to DIR/restored_points.npy (float32)")
    ap.add_argument("--clouds", type=int, default=N_CLOUDS, help="clouds per GPU per step (default: MN40 test size)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default): every rank restores its own --clouds clouds; strong: ONE array of --clouds clouds is "
                         "sharded over the ranks (BASELINE configs #3 / #5: one .npz over 8 GPUs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--streamed", action="store_true",
                    help="time the K passes as a STREAM of K files (pre-processing of file n + 1 on a second HIP stream under file n's "
                         "optimiser tail) instead of one file at a time with a synchronisation after each (the default: BASELINE configs[1])")
    ap.add_argument("--no-overlap", action="store_true", help="(kept for scripts: the default since round 5) one file at a time")
    ap.add_argument("--no-extras", action="store_true", help="skip the bounded side measurements (reference-style unfused "
                    "GPU baseline, ONet-Opt, ONet-Mesh) that ride along in the N = 1 --full line")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU work: initialise the process group (gloo on a CPU host), shard the clouds, push a placeholder "
                         "of every rank's shard through the real gather, print the JSON line with value null - checks the launch "
                         "line, the sharding arithmetic and the line's fields for any --gpus N without N GPUs")
    ap.add_argument("--workload", choices=("convonet-opt", "onet-opt"), default="convonet-opt",
                    help="convonet-opt = the BASELINE metric (default); onet-opt = the ONet-Opt decoder variant "
                         "(BASELINE config #1 model, SURVEY N4) at 500 iterations - an extra line, not the headline")
    ap.add_argument("--backend", default=None, help="TEST ONLY: torch.distributed backend (default: nccl = RCCL on GPUs); 'gloo' lets two "
                    "ranks share ONE GPU (tests/test_gpu_two_processes.py runs the N > 1 code path of this script that way)")
    ap.add_argument("--device", default=None, help="TEST ONLY: the device of every rank (default: cuda:LOCAL_RANK)")
    ap.add_argument("--profile-precision", choices=("f32", "bf16x6", "bf16x3"), default="f32",
                    help="PROFILING ONLY (scripts/pmc_bench.sh): run the timed passes in a split-precision mode; the line is then labelled "
                         "as such in metric / dtype / config.arith and is not the BASELINE metric")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    a.no_overlap = not a.streamed
    onet = a.workload == "onet-opt"
    if onet and a.clouds == N_CLOUDS:
        a.clouds = 256                                                  # one cloud per CU; ~3 s per step

    import ifdefense_amd as I
    from ifdefense_amd import dist as D
    import torch.distributed as dist

    rank, world, local = D.init_from_env("gloo" if a.dry_run else a.backend)
    if world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run for N > 1)" % (a.gpus, world))
    total = a.clouds * world if a.scaling == "weak" else a.clouds
    lo, hi, per = D.shard_range(total, rank, world)
    if a.dry_run:
        # every rank contributes a placeholder of its shard's shape, stamped with the global cloud indices it owns: the
        # gathered array must be 0 ... total - 1 in order on every rank (the sharding helper + the one collective of the path)
        mine = torch.arange(lo, hi, dtype=torch.float32)[:, None, None].expand(hi - lo, 1, 3).contiguous()
        full = D.gather_shards(mine, total, per)
        ok = full.shape == (total, 1, 3) and bool(torch.equal(full[:, 0, 0], torch.arange(total, dtype=torch.float32)))
        if rank == 0:
            print(json.dumps({
                "metric": "restored clouds/sec (1024-pt ModelNet40, %s 500 iters)" % ("ONet-Opt" if onet else "ConvONet-Opt"),
                "value": None, "unit": "clouds/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": None,
                "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "dry_run": True, "gather_ok": ok,
                "config": {"clouds_per_gpu": per, "clouds_total": total, "points": K_POINTS, "adam_steps": ITERATIONS + 1,
                           "parallelism": "shard%d+allgather" % world, "shard_of_rank0": [lo, hi]}}))
        D.shutdown()
        if not ok:
            raise SystemExit("dry run: the gathered array is not the concatenation of the ranks' shards")
        return
    dev = torch.device(a.device) if a.device else torch.device("cuda", local)
    torch.cuda.set_device(dev)

    def reduce_max(seconds):
        """max over the ranks of a host-side duration (RCCL reduces device tensors, gloo host tensors)"""
        if not dist.is_initialized():
            return float(seconds)
        t = torch.tensor([seconds], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())
    my_clouds = synth_clouds(hi - lo, start=lo)                         # every rank synthesises only its own shard
    x = torch.from_numpy(my_clouds).to(dev)                             # resident in HBM before timing
    if onet:
        r = I.OnetRestorer(I.weights.pack_state_dict(I.weights.onet_random_state_dict(0), "onet"), device=dev)
        args = I.DefenseArgs(iterations=ITERATIONS, seed=1234, input_npoint=300, precision=a.profile_precision)
        flop_per_cloud = 2 * 2 * (10 * 256 * 256 + 4 * 256) * K_POINTS * (ITERATIONS + 1)     # 1.347 TFLOP
    else:
        r = I.Restorer(I.weights.pack_state_dict(I.weights.random_state_dict(0)), device=dev)
        # the headline is f32 whatever the environment says: the precision is passed explicitly (--profile-precision only for profiling runs)
        args = I.DefenseArgs(iterations=ITERATIONS, seed=1234, precision=a.profile_precision)
        flop_per_cloud = FLOP_DENSE_PER_CLOUD

    # time the dominant kernel (the persistent optimiser) with events on the stream it is launched on
    ev = []
    orig = r.optimize_points

    def timed_optimize(*p, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(*p, **k)
        e1.record()
        ev.append((e0, e1, out.shape[0]))
        return out

    r.optimize_points = timed_optimize

    gev = []

    def run_steps(k):
        """k passes of the whole path over the resident batch, driven as a stream of k files: the pre-processing of pass
        n + 1 (SOR, preprocess, encoder: ~105 ms of full-GPU work) is enqueued on a second HIP stream behind pass n's
        optimiser launch and runs on the CUs its last round leaves idle (pipeline.defend_stream).  Nothing is skipped or
        cached: every pass recomputes everything from the raw clouds."""
        full = None
        for local_out in I.defend_stream(r, [x] * k, args, bases=[lo] * k, totals=[total] * k, overlap=not a.no_overlap):
            g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            g0.record()
            full = D.gather_shards(local_out, total, per)               # the one collective of the path (RCCL all-gather)
            g1.record()
            gev.append((g0, g1))
            if a.no_overlap:
                torch.cuda.synchronize()                                # one file at a time: its result is complete before the next starts
        return full

    def barrier():
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    if a.warmup > 0:
        out = run_steps(a.warmup)
    ev.clear()
    gev.clear()
    barrier()
    t0 = time.perf_counter()
    out = run_steps(a.steps)
    barrier()
    dt = reduce_max(time.perf_counter() - t0)
    assert out.shape == (total, K_POINTS, 3) and bool(torch.isfinite(out).all())
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, out)

    kern_ms = [e0.elapsed_time(e1) for e0, e1, _ in ev]
    kern_clouds = [n for _, _, n in ev]
    main_ev = list(ev)
    # BASELINE configs #3 / #5 are ONE file over the GPUs of a node (strong scaling).  A weak-scaling run with more than one rank
    # therefore times that too, right behind the headline passes: ONE array of --clouds clouds sharded over the ranks (round-5 verdict)
    strong = None
    if a.full and world > 1 and a.scaling == "weak" and not onet:
        s_lo, s_hi, s_per = D.shard_range(a.clouds, rank, world)
        xs = x[:max(0, s_hi - s_lo)]

        def strong_steps(k):
            out_ = None
            for local_out in I.defend_stream(r, [xs] * k, args, bases=[s_lo] * k, totals=[a.clouds] * k, overlap=False):
                out_ = D.gather_shards(local_out, a.clouds, s_per)
                torch.cuda.synchronize()
            return out_

        strong_steps(1)
        barrier()
        t1 = time.perf_counter()
        so = strong_steps(a.steps)
        barrier()
        t_strong = reduce_max(time.perf_counter() - t1)
        assert so.shape == (a.clouds, K_POINTS, 3)
        strong = {"value": round(a.clouds * a.steps / t_strong, 2), "unit": "clouds/s", "scaling": "strong",
                  "clouds_total": a.clouds, "clouds_per_gpu": s_per, "ms_per_step": round(t_strong / a.steps * 1e3, 2),
                  "what": "ONE %d-cloud array sharded over the %d ranks (BASELINE configs #3 / #5), %d passes timed like the headline "
                          "(barrier + synchronize on both sides, max over ranks); the shard's partial round is split over 2 / 4 CUs per cloud" %
                          (a.clouds, world, a.steps)}
    ev[:] = main_ev
    if rank == 0:
        avg_ms = sum(kern_ms) / len(kern_ms)
        avg_clouds = sum(kern_clouds) / len(kern_clouds)
        achieved = flop_per_cloud * avg_clouds / (avg_ms * 1e-3) / 1e12
        # HBM bytes per launch from the PMC passes (scripts/collect_profiles.sh; counters cannot be read inside this run):
        # quoted only if they were measured on THIS kernel (source hash) and this launch size, else null
        # a file is one launch, or two (pipeline.defend_stream tail_first: the partial round, then the whole rounds); `achieved` is
        # over ALL launches of the kernel (what rocprofv3's per-kernel average corresponds to), the shapes are listed next to it
        launches_per_file = len(kern_ms) / float(a.steps)
        launch_shapes = launch_shapes_of(ev, flop_per_cloud)
        traffic, traffic_src, traffic_shapes = (None, None, None)
        if not onet:
            traffic, traffic_src, traffic_shapes = traffic_from_profiles(a.profile_precision, sum(kern_clouds) / float(a.steps), launches_per_file)
        res = {
            "metric": "restored clouds/sec (1024-pt ModelNet40, %s 500 iters)" % ("ONet-Opt" if onet else "ConvONet-Opt"),
            "value": round(total * a.steps / dt, 2), "unit": "clouds/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 2), "higher_is_better": True,
            "scaling": a.scaling, "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s on ModelNet40-test-like .npz: %d clouds/GPU x 1024 pts, --iterations=500 "
                                   "(501 Adam steps), SOR on, batch_size 192; SOR+preprocess+encode+init+optimise+"
                                   "normalise+gather" % ("ONet-Opt" if onet else "ConvONet-Opt", per),
                       "clouds_per_gpu": per, "clouds_total": total, "points": K_POINTS, "adam_steps": ITERATIONS + 1,
                       "parallelism": "shard%d+allgather" % world, "weights": "seeded random (seed 0)",
                       "driver": "stream of %d files: pre-processing of file n+1 on a second HIP stream under file n's optimiser tail" % a.steps
                                 if not a.no_overlap else "one file at a time, device synchronisation after every file (BASELINE configs[1] literally); inside a file the clouds of its "
                                 "partial last round go first and the other clouds' pre-processing runs under that round (pipeline.defend_stream tail_first)",
                       "arith": "f32 throughout; decoder layers on v_mfma_f32_16x16x4_f32 (bit-equal to an fmaf chain); repulsion terms' "
                                "sqrt / 1/h / 1/d / exp through the 1-ulp hardware instructions (IFD_EXACT_REP off; libifd_exact.so has the "
                                "IEEE expansions, +1.3 %); ReLU'(+0.0) passes in the hot tile (DESIGN section 9); the 5-NN sets of the repulsion "
                                "term are EXACT (direct differences, ties by index) where the reference's expanded-form float32 ranking swaps "
                                "near-ties and keeps 'self' for pairs closer than ~1.5e-4 - ifd_opt_params.knn_reference_form reproduces that bug "
                                "for bug (validation mode: with it config #5 K = 256 meets the 1e-3 bound inside the oracle's own 1-ulp floor, "
                                "without it 7 of 4096 points exceed it after 10 steps; DESIGN section 9); the optimised points of a cloud are "
                                "processed in Morton order of their initial coordinates (the reference's draw order is i.i.d.)"},
            "roofline": {"bound": "mfma", "kernel": "ifd::onet_optimize_kernel" if onet else "ifd::optimize_kernel",
                         "achieved": round(achieved, 2),
                         "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / F32_MFMA_PEAK_TFLOPS, 4),
                         "traffic": traffic, "traffic_source": traffic_src, "traffic_launch_shapes": traffic_shapes, "launch_ms": round(avg_ms, 2),
                         "clouds_per_launch": avg_clouds, "flop_per_cloud": flop_per_cloud,
                         "launches_per_file": launches_per_file, "launch_shapes": launch_shapes},
            "optimise_only_clouds_per_s": round(sum(kern_clouds) / (sum(kern_ms) * 1e-3), 2),
            "gather_ms": round(sum(g0.elapsed_time(g1) for g0, g1 in gev) / max(1, len(gev)), 3),
        }
        if strong is not None:
            res["strong_scaling"] = strong
        if a.profile_precision != "f32":
            # a profiling run of the opt-in split-precision mode: labelled so that it cannot be read as the BASELINE metric
            res["metric"] += " [PROFILING RUN, decoder layers %s - not the headline]" % a.profile_precision
            res["dtype"] = "%s (%s)" % (a.profile_precision, "f32-equivalent split" if a.profile_precision == "bf16x6" else "REDUCED precision")
            res["config"]["arith"] = ("decoder dense layers as %s bf16 products on v_mfma_f32_16x16x32_bf16 (ifd_opt_params.precision, "
                                      "csrc/tile_bf.h); everything else f32" % ("six" if a.profile_precision == "bf16x6" else "three"))
            res["roofline"]["note"] = "achieved is in f32-EQUIVALENT FLOP against the f32-MFMA peak; the matrix core executes %dx as many bf16 FLOP" % \
                (6 if a.profile_precision == "bf16x6" else 3)
        streamed = None
        if a.full and world == 1 and not onet and not a.no_extras and a.no_overlap:
            # the same passes as a stream of files (what a directory of .npz files through the CLI does): five passes, driver-timed
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in I.defend_stream(r, [x] * 8, args, bases=[lo] * 8, totals=[total] * 8, overlap=True):
                pass
            torch.cuda.synchronize()
            dt1 = (time.perf_counter() - t1) / 8
            streamed = {"value": round(total / dt1, 2), "unit": "clouds/s", "ms_per_file": round(dt1 * 1e3, 2),
                        "what": "the same workload driven as a stream of 8 files: pre-processing of file n+1 on a second HIP stream under "
                                "file n's last optimiser round (a directory input of the CLI); the first file has nothing to hide under"}
        if a.full and world == 1 and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(my_clouds, onet=onet, full_run_clouds=0 if onet else 4)
            if not onet:
                res["cpu_baseline"]["host_saturating"] = cpu_baseline_saturating(res["cpu_baseline"])
                res["cpu_baseline"] = cpu_baseline_pick(res["cpu_baseline"])
        if a.full and world == 1 and not onet and not a.no_extras:
            res["extras"] = extras(dev)
            if streamed is not None:
                res["extras"]["streamed"] = streamed
            try:
                res["f32_equivalent"] = f32_equivalent_block(r, x, args, lo, total, ev)
            except Exception as e:      # noqa: BLE001
                res["f32_equivalent"] = {"error": str(e)[:200]}
            res["extras"]["split_precision"] = split_precision_extras(r, x, args, lo, total, ev)
            try:
                res["extras"]["trained_like_full"] = trained_like_full(dev)
            except Exception as e:      # noqa: BLE001
                res["extras"]["trained_like_full"] = {"error": str(e)[:200]}
        print(json.dumps(res))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
