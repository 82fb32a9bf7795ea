#!/usr/bin/env python
"""bench.py — sliding-window solves/sec (10 KF, 150 features) + feature-select ms/frame on MI355X.

A "step" is one pass of the hot path over one batch of synthetic EuRoC-shaped inputs that are
already resident in HBM: avm_window_solve_batch() over `--windows` independent 11-frame windows
per GPU (BASELINE.json configs[3]: 4096 windows / GPU; configs[4]: 8 x 4096 = 32768 over 8 GPUs).
Every window of the batch is a DIFFERENT synthetic trajectory (`--distinct` < `--windows` tiles a
smaller set; it is an option, not the default).  Windows shard embarrassingly: rank r owns window ids
[r*W, (r+1)*W); the only collective is one RCCL all-gather of the final poses per step ("weak"
scaling: per-GPU work fixed), issued by the library itself (avm_gather_states, raw rccl.h).

Prints ONE JSON line on rank 0 (see the driver contract in the task statement), with
  roofline     : FP64 FLOP model of the window-solve kernel / its HIP-event duration vs the
                 78.6 TFLOP/s FP64 peak (vector == matrix rate on MI355X); model in DESIGN.md
and, with --full only (a plain run sets up, warms up, times the steps and prints the line):
  cpu_baseline : the CPU oracle ("port" of the reference algorithm, compiled -O3 -march=native on this host)
                 timed on the host cores this process may use: median of >= 5 passes, 1 core and all cores
  feature_select: ms/frame + its own roofline and CPU baseline
  sub-records  : ragged tracks, MARGIN_SECOND_NEW, the extended problem, single-window and host-call latency,
                 the FP64 peak re-measured by scripts/ubench/peak

--dump-outputs DIR writes what the last timed step handed back (solved states, summaries, the new prior) as
DIR/<name>.npy; the inputs depend only on the arguments, so two builds can be compared output for output.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
PKG = "anticipated-vins-mono_amd"

FP64_PEAK_TFLOPS = 78.6  # MI355X datasheet FP64 vector == FP64 matrix; measured: scripts/ubench/peak.hip, profiles/r02_fp64_peak.json
HBM_PEAK_GBS = 8000.0


def flop_model(n_fac, n_feat, summ):
    """Algorithmic FP64 FLOPs of the solves in `summ` (numpy structured summaries). See DESIGN.md §Roofline.
    Jacobian evaluations and linear solves: one at the start + one per successful step (a rejected step re-uses the
    factorization: DoglegStrategy `reuse`), except after a step accepted in the last iteration the options allow - the
    minimizer stops there and neither is ever used; residual-only evaluations: one per step attempt."""
    import numpy as np

    it = summ["num_iterations"].astype(np.float64)
    ns = summ["num_successful"].astype(np.float64)
    lin_solves = np.minimum(1.0 + ns, np.maximum(it, 1.0))
    jac_evals = lin_solves
    per_jac = 1800.0 * n_fac + 5.0e5                       # factor r/J + J^T J blocks, 10 IMU factors + prior
    per_lin = 66.0 * 67.0 * n_feat + 165.0**3 / 3.0 + 2.0 * 165.0**2  # Schur rank-150 update + Cholesky + solves
    per_cand = 230.0 * n_fac + 3.0e4                       # residual-only evaluation
    return float((jac_evals * per_jac + lin_solves * per_lin + it * per_cand).sum())


def flop_models_other(host, n_windows):
    """Algorithmic FP64 FLOPs per launch of the kernels around the solve, from the batch's own counts.
    preint + sqrt_info : per IMU sample the products the sample step NEEDS (round 6, VERDICT r5 6b: the reference's dense 15 x 15 x 15 / 15 x 18 x 18
                         products were priced before, of which a third multiply structural zeros or the identity - F = I + N has three identity
                         columns, V's bias-walk columns are I dt, integration_base.h:90-120): four products over the twelve columns that carry
                         information, F J, P F^T, F (P F^T), V (Q V^T): 4 x 2 x 15 x 12 x 15, + ~600 for the midpoint integration; per interval
                         the 15 x 15 inverse and its LLT (~1.0e4)
    marginalize        : per projection factor of a start-0 feature 2600 (r, J with the ex_pose block, its Gram products), IMU factor 0
                         4.3e4, the old prior 2 n^2 + n^2 (n + 1), one rank-1 update of the 73 x 73 pose block per eliminated depth
                         (73 x 74), the 15 x 15 pseudo-inverse and A' = Arr - T Amr (2.4e5)
    prior_chol         : n^3 / 3 + 2 n^2 at n = 75 (the factor IS the square root; the certification's inverse is overhead, not counted)"""
    import numpy as np

    a = host.a
    samples = float(a["imu_n"].sum()) * n_windows / a["imu_n"].shape[0]
    preint = samples * (4 * 2 * 15.0 * 12 * 15 + 600.0) + n_windows * 10 * 1.0e4
    nobs, start, nf = a["feat_nobs"], a["feat_start"], a["n_feat"]
    live = np.arange(nobs.shape[1])[None, :] < nf[:, None]
    s0 = live & (start == 0)
    k0 = float(((nobs - 1).clip(min=0) * s0).sum()) * n_windows / nobs.shape[0]
    m0 = float(s0.sum()) * n_windows / nobs.shape[0]
    n = 75.0
    marg = k0 * 2600.0 + m0 * 73.0 * 74.0 + n_windows * (4.3e4 + 2 * n * n + n * n * (n + 1) + 2.4e5)
    chol = n_windows * (n**3 / 3.0 + 2 * n * n)
    return {"preint": preint, "marginalize": marg, "prior_eig": chol}


def kernel_source_sha256():
    """Hash of the sources the window kernels are built from: a committed rocprofv3 --pmc summary (profiles/*_pmc_traffic.json) carries the
    hash it was measured on, and roofline.traffic is only reported from a summary whose hash is the current one."""
    import hashlib

    h = hashlib.sha256()
    for f in ("window_solve.hip", "prior_eig.hip", "preint.hip", "fsel.hip", "kernels.hpp", "devmath.hpp", "Makefile"):
        h.update(open(os.path.join(ROOT, PKG, "csrc", f), "rb").read())
    return h.hexdigest()


def committed_profile():
    """(dict of the newest profiles/*_pmc_traffic.json, its file name, why it cannot be used or None)."""
    pd = os.path.join(ROOT, "profiles")
    tp = sorted(p for p in os.listdir(pd) if p.endswith("_pmc_traffic.json"))
    if not tp:
        return None, None, "no profiles/*_pmc_traffic.json"
    j = json.load(open(os.path.join(pd, tp[-1])))
    have, want = j.get("_kernel_source_sha256"), kernel_source_sha256()
    if have != want:
        return j, tp[-1], (f"profiles/{tp[-1]} was measured on other kernel sources (sha256 {str(have)[:12]}... vs {want[:12]}... now): "
                           "re-run scripts/gpu_profile.sh + scripts/summarize_rocprof.py")
    return j, tp[-1], None


def host_cpus():
    """(threads this process may run on, description): scheduler affinity, capped by the cgroup CPU quota."""
    n_aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    n = n_aff if quota is None else max(1, min(n_aff, int(quota)))
    return n, {"model": model, "os_cpu_count": os.cpu_count(), "sched_affinity": n_aff, "cgroup_cpu_quota": quota}


def native_oracle():
    """The oracle compiled for THIS host's cores (-O3 -march=native); falls back to the portable prebuilt library."""
    import oracle_py

    out = os.path.join(tempfile.gettempdir(), f"libavm_oracle_native_{os.getpid()}.so")
    cmd = ["g++", "-O3", "-march=native", "-std=c++17", "-fPIC", "-pthread", "-shared", "-o", out, os.path.join(ROOT, "oracle", "avm_oracle.cpp")]
    try:
        subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        oracle_py.use_library(out)
        return "g++ -O3 -march=native, compiled on this host"
    except Exception:  # no compiler on the box: the prebuilt x86-64-v3 build
        oracle_py.lib()
        return "prebuilt g++ -O3 -march=x86-64-v3"


def median_rate(fn, units, passes=5, budget_s=12.0):
    """units / median wall time of fn() over >= 3 (normally `passes`) passes, bounded by budget_s of total time."""
    times = []
    t_all = time.perf_counter()
    for k in range(passes):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
        if k >= 2 and time.perf_counter() - t_all > budget_s:
            break
    return units / statistics.median(times), len(times)


def host_call_latency(abi, synth, reps=50):
    """The drop-in calls timed the way the reference makes them (estimator_node.cpp:340,360: one f_selector.select() and one
    estimator.optimization() per image, from HOST members): include/avm_host.hpp's Estimator / FeatureSelector through the ctypes hooks of
    tests/host_cpp.  optimization() = marshal the members + H2D + pre-integration, solve, marginalization, prior square root + D2H + unmarshal;
    select() = split the image, horizon, depth cloud, marshal + H2D + the greedy kernels + D2H.  Median wall time of the call itself
    (std::chrono around it inside the hook), next to the reference's own per-image numbers (results.tex:72-85: 30 ms / 9 ms on its CPU)."""
    import ctypes as C

    import numpy as np

    d = os.path.join(ROOT, "tests", "host_cpp")
    so = os.path.join(d, "libavm_host_shim.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(so)
    L.hs_create.restype = C.c_void_p
    L.hs_last_error.restype = C.c_char_p
    L.hs_last_call_ms.restype = C.c_double
    h = C.c_void_p(L.hs_create(0))
    out = {}
    try:
        w = synth.make_windows(1, tracks="dense")
        ws = w.struct()
        nf = int(w.a["n_feat"][0])
        fid, sf = np.arange(nf, dtype=np.int32), np.ones(nf, np.int32)
        z = np.zeros(1, np.int32)

        def load():
            rc = L.hs_load_window(h, C.byref(ws), 0, abi.iptr(fid), abi.iptr(sf), 0, abi.iptr(z), abi.iptr(z), abi.iptr(z))
            if rc != 0:
                raise RuntimeError(L.hs_last_error().decode())
            L.hs_set_flags(h, 1, 0, 0)  # (the load clears the state: solver_flag = NON_LINEAR, marginalization_flag = MARGIN_OLD again)

        o = abi.default_options()
        L.hs_set_options(h, C.byref(o))
        ms = []
        for _ in range(reps + 5):
            load()  # (the members as the front end leaves them; not timed)
            if L.hs_optimization(h) != 0:
                raise RuntimeError(L.hs_last_error().decode())
            ms.append(L.hs_last_call_ms())
        out["optimization"] = {"value": statistics.median(ms[5:]), "min": min(ms[5:]), "max": max(ms[5:]), "reps": reps,
                               "what": "avm_host::Estimator::optimization() on one dense 11-frame window (150 features, 1500 factors, prior, MARGIN_OLD) from host "
                                       "members: marshal + H2D + 5 launches + D2H + unmarshal", "reference_cpu_ms": 30.0,
                               "reference_source": "support_files/paper results.tex:82 (Ceres, the reference's own machine)"}
        # ---- select(): 500 new candidates per image, 150 selected, horizon 10 (BASELINE.json configs[2]) against the loaded window's depth cloud
        load()
        cam = synth.CAM
        camv = np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")], float)
        L.hs_sel_create(h, abi.dptr(camv), int(cam["image_width"]), int(cam["image_height"]), 10)
        L.hs_sel_set_parameters(h, C.c_double(synth.ACC_N), C.c_double(synth.ACC_W), 1, 150, 10, 0)
        rng = np.random.default_rng(11)
        pose10, sb10 = w.a["pose"][0, 10], w.a["speedbias"][0, 10]
        cap = 8192
        io, tr, se = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ni, nt = C.c_int32(0), C.c_int32(0)
        ms, nsel, next_id, stamp, parts = [], [], 1, 10.0, []
        for _ in range(reps + 5):
            ids = np.arange(next_id, next_id + 500, dtype=np.int32)
            next_id += 500
            u, v = rng.uniform(0, cam["image_width"], 500), rng.uniform(0, cam["image_height"], 500)
            rows = np.zeros((500, 8))
            rows[:, 0], rows[:, 1], rows[:, 2] = (u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], 1.0
            rows[:, 3], rows[:, 4], rows[:, 7] = u, v, rng.uniform(0.05, 1.0, 500).astype(np.float32)
            P, Q = pose10[:3] + rng.normal(0, 0.05, 3), pose10[3:] + rng.normal(0, 0.01, 4)
            Q /= np.linalg.norm(Q)
            vecs = [np.ascontiguousarray(x, float) for x in (P, Q, sb10[:3] + rng.normal(0, 0.05, 3), rng.normal(0, 0.5, 3) + [0, 0, 9.8], rng.normal(0, 0.1, 3), sb10[3:6])]
            L.hs_sel_set_next_state(h, C.c_double(stamp), *[abi.dptr(x) for x in vecs])
            rc = L.hs_sel_select(h, 500, abi.iptr(ids), abi.dptr(rows), C.c_double(stamp), 20, abi.iptr(io), C.byref(ni), abi.iptr(tr), C.byref(nt), abi.iptr(se), cap)
            if rc < 0:
                raise RuntimeError(L.hs_last_error().decode())
            ms.append(L.hs_last_call_ms())
            nsel.append(rc)
            pt = (C.c_double * 3)()
            L.hs_sel_last_parts_ms(h, pt)
            parts.append((pt[0], pt[1], pt[2]))
            stamp += 0.1
        out["select"] = {"value": statistics.median(ms[5:]), "min": min(ms[5:]), "max": max(ms[5:]), "reps": reps, "selected_per_call": int(statistics.median(nsel[5:])),
                         "device_calls_ms": {k: statistics.median(p[i] for p in parts[5:]) for i, k in enumerate(("horizon_imu", "depth_cloud_incl_marshal", "select_batch"))},
                         "what": "avm_host::FeatureSelector::select() on an image of 500 new features, maxFeatures 150, horizon 10, IMU horizon, the window's "
                                 "depth cloud: split + horizon + marshal + H2D + greedy kernels + D2H", "reference_cpu_ms": 9.0,
                         "reference_source": "support_files/paper results.tex:72-85 (the reference's lazy greedy on its own machine)"}
    finally:
        L.hs_destroy(h)
    return out


def free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks ourselves - one process per GPU with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set as torch.distributed.run would set them -, relay rank 0's
    stdout (the JSON line), send every other rank's output to stderr, and exit non-zero if ANY rank fails (the others are
    then terminated by process group, never by pattern)."""
    import signal

    port = int(os.environ.get("MASTER_PORT", 0)) or free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), AVM_BENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # this host driver only supports dmabuf IPC (RCCL across processes)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, start_new_session=True,
                                      stdout=(subprocess.PIPE if r == 0 else sys.stderr)))
    import threading

    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    failed = None
    try:
        pending = set(range(n))
        t_rank0_done = None
        while pending and failed is None:
            for r in sorted(pending):
                rc = procs[r].poll()
                if rc is not None:
                    pending.discard(r)
                    if rc != 0:
                        failed = (r, f"exit code {rc}")
                    elif r == 0:
                        t_rank0_done = time.time()
            if failed is None and t_rank0_done is not None and pending and time.time() - t_rank0_done > 120.0:
                failed = (min(pending), "still running 120 s after rank 0 finished")
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGTERM)  # exactly the process groups we started
                except ProcessLookupError:
                    pass
        for p in procs:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
    reader.join(timeout=10)
    out0 = b"".join(c for c in chunks if c)
    sys.stdout.write(out0.decode(errors="replace"))
    sys.stdout.flush()
    if failed is not None:
        print(f"[bench] rank {failed[0]} failed ({failed[1]}); the other ranks were stopped", file=sys.stderr)
        raise SystemExit(1)
    raise SystemExit(0)


def launch_check(rank, world):
    """--launch-check: the rendezvous of the N ranks and the max-over-ranks reduction of the timing, on gloo, BEFORE anything
    touches HIP - what the CPU tier can test of `bench.py --gpus N` (tests/test_bench_launch.py)."""
    import torch
    import torch.distributed as dist

    if os.environ.get("AVM_BENCH_FAIL_RANK") == str(rank):  # the failure leg of the launcher test
        raise SystemExit(7)
    ranks = [rank]
    tmax = float(rank + 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, torch.tensor([rank], dtype=torch.int64))
        ranks = [int(g.item()) for g in got]
        t = torch.tensor([tmax], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tmax = float(t.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": world, "ranks": ranks, "max_over_ranks": tmax,
                          "self_launched": bool(os.environ.get("AVM_BENCH_SELF_LAUNCHED"))}))


DUMP_SEED = 0
DUMP_ROWS_BYTES = 36_000_000      # the solved states, the summaries and the prior's small members
DUMP_PRIOR_J_BYTES = 20_000_000   # the prior's 96 x 96 factor (74 KB a window): at most 256 windows of it
DUMP_GATHERED_BYTES = 4_000_000   # N > 1: the all-gathered poses


def _dump_rows(n, keep, seed):
    """Row indices 0..n-1, or a sorted sample of `keep` of them drawn with a fixed seed when keep < n."""
    import numpy as np

    if keep >= n:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, max(int(keep), 1), replace=False))


def _dump_take(x, rows):
    """x[rows] of a device tensor (indexed on the device) as a float64 host array."""
    import numpy as np
    import torch

    return np.ascontiguousarray(x[torch.as_tensor(rows, device=x.device)].cpu().numpy(), dtype=np.float64)


def dump_outputs(d, win, summ, prior, gathered):
    """--dump-outputs: what a caller of the timed path receives from its last step, as d/<name>.npy (float64, under 64 MB in all):
    the solved states (pose, speedbias, ex_pose, inv_depth), every field of the per-window summaries (summary_<field>), the new
    prior when the marginalization runs (prior_<member>) and, with N > 1, the all-gathered poses (pose_gathered).  The inputs
    depend only on the arguments.  A batch too large for the budget is written for a seeded sample of its windows, listed in
    windows.npy; prior_J is always such a sample (prior_J_windows.npy), pose_gathered when it is large (pose_gathered_rows.npy)."""
    import numpy as np

    buffers = importlib.import_module(PKG + ".buffers")
    os.makedirs(d, exist_ok=True)
    W = win.n_windows
    full = np.arange(W)
    out = {k: _dump_take(win.a[k], full) for k in ("pose", "speedbias", "ex_pose", "inv_depth")}
    s = buffers.summary_to_numpy(summ)
    for f in s.dtype.names:
        out["summary_" + f] = np.ascontiguousarray(s[f], dtype=np.float64)
    if prior is not None:
        out.update({"prior_" + k: _dump_take(v, full) for k, v in prior.a.items() if k != "J"})
    rows = _dump_rows(W, DUMP_ROWS_BYTES // sum(v[0].nbytes for v in out.values()), DUMP_SEED)
    if len(rows) < W:
        out = {k: v[rows] for k, v in out.items()}
        out["windows"] = rows.astype(np.float64)
    if prior is not None:
        J = prior.a["J"]
        jr = _dump_rows(W, min(256, DUMP_PRIOR_J_BYTES // (J[0].numel() * 8)), DUMP_SEED + 1)
        out["prior_J"] = _dump_take(J, jr)
        out["prior_J_windows"] = jr.astype(np.float64)
    if gathered is not None:
        gr = _dump_rows(gathered.shape[0], DUMP_GATHERED_BYTES // (gathered[0].numel() * 8), DUMP_SEED + 2)
        out["pose_gathered"] = _dump_take(gathered, gr)
        if len(gr) < gathered.shape[0]:
            out["pose_gathered_rows"] = gr.astype(np.float64)
    for k, v in out.items():
        np.save(os.path.join(d, k + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--windows", type=int, default=4096, help="windows per GPU per step")
    ap.add_argument("--distinct", type=int, default=0, help="distinct generated windows per rank, tiled up to --windows (0 = all distinct)")
    ap.add_argument("--gen-procs", type=int, default=0, help="worker processes generating the synthetic windows (0 = one per usable CPU; 1 = in-process, for runs under a profiler)")
    ap.add_argument("--tracks", default="dense", choices=["dense", "sparse"])
    ap.add_argument("--fsel-problems", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fsel", action="store_true")
    ap.add_argument("--no-host-latency", action="store_true", help="skip latency_host_call_ms (the C++ host objects of include/avm_host.hpp through tests/host_cpp)")
    ap.add_argument("--no-extras", action="store_true", help="skip the sub-records (ragged tracks, single-window latency, selector at HORIZON 13)")
    ap.add_argument("--gather", default="library", choices=["library", "torch"], help="who issues the all-gather of the final poses (N > 1)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend for N > 1.  gloo: the ranks may share a "
                    "device (LOCAL_RANK modulo the visible devices) and the poses are gathered through the host - for exercising the N > 1 path "
                    "end to end on a box with fewer GPUs than ranks (RCCL refuses two ranks on one device); never the configuration to quote")
    ap.add_argument("--launch-check", action="store_true", help="rendezvous of the N ranks on gloo and exit, before HIP is initialised")
    ap.add_argument("--full", action="store_true", help="also measure what the headline figure does not need: the sub-records, the feature "
                    "selector, the CPU baseline and the FP64 peak (the --no-* options thin this out)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the last step's outputs as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus, sys.argv[1:])  # never returns

    import numpy as np

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus N` (it spawns "
                         f"its own ranks) or under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`")
    if args.launch_check:
        return launch_check(rank, world)
    ncpu, cpu_info = host_cpus()

    abi = importlib.import_module(PKG + ".abi")
    synth = importlib.import_module(PKG + ".synth")
    buffers = importlib.import_module(PKG + ".buffers")

    # ---- inputs: generated on-rank from (seed, window id) on the host cores (worker processes are forked BEFORE the HIP
    #      runtime is initialised), then resident in HBM
    W = args.windows
    n_distinct = W if args.distinct <= 0 else min(args.distinct, W)
    t_gen = time.perf_counter()
    base = synth.make_windows_parallel(n_distinct, first_id=rank * W, tracks=args.tracks, procs=args.gen_procs or max(1, min(64, ncpu // max(world, 1))))
    host = base if n_distinct == W else synth.tile_windows(base, W)
    t_gen = time.perf_counter() - t_gen
    extras = world == 1 and args.full and not args.no_extras and not args.launch_check
    sparse_base = None
    if extras and args.tracks == "dense":
        # the ragged-track sub-record (a quarter of the batch generated, tiled: it is a sub-record, the headline batch is all distinct)
        sparse_base = synth.make_windows_parallel(min(W, 1024), first_id=rank * W, tracks="sparse", procs=args.gen_procs or max(1, min(64, ncpu)))

    import torch

    dist = None
    if world > 1:
        import torch.distributed as dist  # noqa: F811

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "gloo":
            if torch.cuda.is_available():
                local_rank = local_rank % torch.cuda.device_count()
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"

    est_m = importlib.import_module(PKG + ".estimator")
    fs_m = importlib.import_module(PKG + ".feature_selector")
    lib_m = importlib.import_module(PKG + ".lib")

    opt = abi.default_options()
    opt.marginalization_flag = abi.MARGIN_NONE if os.environ.get("AVM_BENCH_NO_MARG") else opt.marginalization_flag
    ctx = lib_m.Context(local_rank)
    E = est_m.Estimator(ctx=ctx, options=opt)

    n_fac = float((host.a["feat_nobs"] - 1).clip(min=0).sum(1).mean())
    n_feat = float(host.a["n_feat"].mean())
    win = host.to_device(dev)
    pristine = {k: win.a[k].clone() for k in ("pose", "speedbias", "ex_pose", "inv_depth")}
    gathered = torch.empty((world * W, 11, 7), dtype=torch.float64, device=dev) if world > 1 else None
    use_lib_gather = world > 1 and args.gather == "library" and hasattr(ctx, "gather_states") and args.backend == "nccl"
    gather_checked = False
    gloo = world > 1 and args.backend == "gloo"
    if use_lib_gather:
        # the library's own communicator (raw rccl.h, avm_comm_*): the 128-byte unique id travels over torch.distributed
        uid = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            uid = torch.frombuffer(bytearray(ctx.comm_unique_id()), dtype=torch.uint8).clone()
        uid = uid.to(dev)
        dist.broadcast(uid, 0)
        ok = 1
        try:
            ctx.comm_init(world, rank, bytes(uid.cpu().numpy().tobytes()))
        except Exception as e:  # keep the job alive: every rank falls back to torch.distributed together
            ok = 0
            print(f"[bench] rank {rank}: avm_comm_init failed ({e}); falling back to torch.distributed", file=sys.stderr)
        flag = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        use_lib_gather = bool(flag.item())
        if use_lib_gather:
            # one untimed self-check of the library's collective against torch.distributed's on the same buffer: a rank that gets
            # an error or different bytes sends every rank to the torch.distributed gather together
            ok = 1
            try:
                probe = torch.arange(W * 77, dtype=torch.float64, device=dev).reshape(W, 11, 7) + rank * 1.0e6
                want = torch.empty_like(gathered)
                ctx.gather_states(probe, gathered, W * 77)
                torch.cuda.synchronize()
                dist.all_gather_into_tensor(want, probe)
                ok = int(torch.equal(want, gathered))
            except Exception as e:
                ok = 0
                print(f"[bench] rank {rank}: avm_gather_states self-check failed ({e}); falling back to torch.distributed", file=sys.stderr)
            flag = torch.tensor([ok], dtype=torch.int32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            use_lib_gather = bool(flag.item())
            gather_checked = use_lib_gather

    marg = opt.marginalization_flag != abi.MARGIN_NONE
    prior_slots = buffers.PriorOutArrays.alloc(W, win.dims["max_prior"], win.dims["max_pblk"], dev) if marg else None

    summ_slots = buffers.summary_alloc(W, dev)  # (handed back in like the prior's slots: no allocation or fill inside a step)
    restore_dst, restore_src = [win.a[k] for k in pristine], list(pristine.values())

    def step():
        # (torch's copies run on the legacy default stream; the ctx stream is a blocking stream, so the solve is ordered
        #  after them and the next step's copies after the solve: include/avm.h "stream ordering")
        # the batch's states back to the unsolved ones (the stand-in for the next batch arriving): one launch for the four arrays
        if hasattr(torch, "_foreach_copy_"):
            torch._foreach_copy_(restore_dst, restore_src)
        else:
            for k, v in pristine.items():
                win.a[k].copy_(v)
        summ = E.optimization(win, want_summary=True, prior_out=prior_slots, summary_out=summ_slots)
        if world > 1:
            if use_lib_gather:
                ctx.gather_states(win.a["pose"], gathered, W * 77)
            elif gloo:  # (through the host: gloo has no device collectives)
                hg = torch.empty(world * W * 77, dtype=torch.float64)
                dist.all_gather_into_tensor(hg, win.a["pose"].cpu().reshape(-1))
                gathered.copy_(hg.view(world * W, 11, 7))
            else:
                dist.all_gather_into_tensor(gathered, win.a["pose"])
        return summ

    kernel_ms, all_ms, summ = [], {k: [] for k in ("preint", "window_solve", "marginalize", "prior_eig")}, None
    for _ in range(args.warmup):
        summ = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        summ = step()
        kernel_ms.append(ctx.kernel_ms("window_solve"))
        for k in all_ms:
            all_ms[k].append(ctx.kernel_ms(k))
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if gloo else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    value = world * W * args.steps / elapsed
    per_rank_solve_ms = [float(np.mean(kernel_ms))]
    per_rank_gather_ms = None
    if world > 1:  # every rank's own solve-kernel time (HIP events on its ctx stream) and its last gather, for the scaling record
        pr = torch.tensor([float(np.mean(kernel_ms)), ctx.kernel_ms("gather_states") if use_lib_gather else -1.0], dtype=torch.float64, device="cpu" if gloo else dev)
        allr = torch.empty(world * 2, dtype=torch.float64, device="cpu" if gloo else dev)
        dist.all_gather_into_tensor(allr, pr)
        allr = allr.view(world, 2)
        per_rank_solve_ms = [float(x) for x in allr[:, 0].cpu()]
        per_rank_gather_ms = [float(x) for x in allr[:, 1].cpu()] if use_lib_gather else None
    if args.dump_outputs and rank == 0:  # (before the --full records, which reuse the prior's slots)
        dump_outputs(args.dump_outputs, win, summ, prior_slots, gathered)

    result = None
    if rank == 0:
        s = buffers.summary_to_numpy(summ)
        flops = flop_model(n_fac, n_feat, s)
        k_ms = float(np.mean(kernel_ms))
        solve_form = ctx.last_solve_form() if hasattr(ctx, "last_solve_form") else "latency"
        solve_kernel = "window_solve_tp_kernel" if solve_form == "throughput" else "window_solve_kernel"
        marg_form = ctx.last_marg_form() if hasattr(ctx, "last_marg_form") else "latency"
        marg_kernel = "marginalize_tp_kernel" if marg_form == "throughput" else "marginalize_kernel"
        achieved = flops / (k_ms * 1e-3) / 1e12
        traffic, traffic_src, mfma_util, fabric_gbs, wait_any = None, None, None, None, None
        prof_j, prof_name, prof_err = committed_profile()  # newest committed rocprofv3 --pmc summary, if it belongs to these kernel sources
        if prof_err:
            traffic_src = "UNAVAILABLE: " + prof_err
            print("[bench] roofline.traffic not reported: " + prof_err, file=sys.stderr)
        elif W == 4096 and args.tracks == "dense" and opt.marginalization_flag == abi.MARGIN_OLD:
            # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_* passes of this same command (scripts/gpu_profile.sh), per launch
            tj = prof_j.get(solve_kernel)
            if tj is None:
                prof_err = f"profiles/{prof_name} has no entry for {solve_kernel}"
                traffic_src = "UNAVAILABLE: " + prof_err
                tj = {"traffic_bytes_per_launch": None}
            traffic = tj["traffic_bytes_per_launch"]
            mfma_util, fabric_gbs, wait_any = tj.get("mfma_util"), tj.get("fabric_GBs"), tj.get("wait_any_frac")
            traffic_src = (f"profiles/{prof_name}: (2*FETCH_SIZE + WRITE_SIZE) KB per launch, separate --pmc passes; mfma_util = SQ_VALU_MFMA_BUSY_CYCLES / "
                           "(dispatch ns x 2.4 GHz x 1024 SIMDs); measured on the kernel sources this run was built from (sha256 checked)")
        alg_bytes = W * (44.0 * n_fac + 23.0e3 + 45.6e3 + 3.0e3 + 2.6e3)  # ~140 KB / solve at K=1500
        # the FP64 peak of THIS device, re-measured in a --full run when the micro-benchmark is built (scripts/ubench/peak, made by
        # __graft_entry__.build()); else the committed measurement of round 2
        peak_meas = None
        pk = os.path.join(ROOT, "scripts", "ubench", "peak")
        if os.path.exists(pk) and args.full and not args.no_extras:
            try:
                out = subprocess.run([pk], capture_output=True, text=True, timeout=120).stdout
                peak_meas = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
                if "error" in peak_meas:
                    peak_meas = None
                else:
                    peak_meas["measured_in_this_run"] = True
            except Exception as e:  # noqa
                print(f"[bench] scripts/ubench/peak failed: {e}", file=sys.stderr)
        pm = os.path.join(ROOT, "profiles", "r02_fp64_peak.json")
        if peak_meas is None and os.path.exists(pm):
            peak_meas = json.load(open(pm))
        # ---- the kernels around the solve: the same roofline entry each (FLOP models: flop_models_other; counters: the committed profile)
        other = flop_models_other(host, W)
        kernels = {}
        for key, names in (("preint", ("preint_kernel", "sqrt_info_kernel")), ("marginalize", (marg_kernel,)),
                           ("prior_eig", ("prior_chol_kernel", "prior_eig_kernel"))):
            ms_k = float(np.mean(all_ms[key])) if all_ms[key] else 0.0
            if ms_k <= 0.0:
                continue
            ach = other[key] / (ms_k * 1e-3) / 1e12
            ent = {"kernels": list(names), "kernel_ms": ms_k, "flops_per_launch": other[key], "achieved": ach, "unit": "TFLOP/s",
                   "peak": FP64_PEAK_TFLOPS, "frac": ach / FP64_PEAK_TFLOPS, "bound": "mfma"}
            if prof_j is not None and not prof_err and W == 4096 and args.tracks == "dense":
                pj = prof_j.get(names[0])
                if pj:
                    ent.update({"traffic": pj.get("traffic_bytes_per_launch"), "mfma_util": pj.get("mfma_util"), "wait_any_frac": pj.get("wait_any_frac"),
                                "fabric_GBs": pj.get("fabric_GBs")})
            kernels[key] = ent
        kernels["window_solve"] = {"kernels": [solve_kernel], "kernel_ms": k_ms, "flops_per_launch": flops, "achieved": achieved, "unit": "TFLOP/s",
                                   "peak": FP64_PEAK_TFLOPS, "frac": achieved / FP64_PEAK_TFLOPS, "bound": "mfma", "traffic": traffic,
                                   "mfma_util": mfma_util, "wait_any_frac": wait_any, "fabric_GBs": fabric_gbs}
        furthest = min(kernels.items(), key=lambda kv: kv[1]["frac"])[0]
        result = {
            "metric": "sliding-window solves/sec (10 KF, 150 feats)",
            "value": value,
            "unit": "solves/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"{W} independent 11-frame windows per GPU, {int(n_feat)} features, {int(n_fac)} projection factors "
                            f"({args.tracks} tracks), 10 IMU factors (200 Hz raw samples pre-integrated on device), 75-dim prior, "
                            f"max_num_iterations=8, no time cap; BASELINE.json configs[3] (x{world} GPUs = configs[4] shape)",
                "windows_per_gpu": W,
                "distinct_windows_per_gpu": int(base.n_windows),
                "marginalization": "MARGIN_OLD" if opt.marginalization_flag == abi.MARGIN_OLD else "none",
                "mean_iterations": float(s["num_iterations"].mean()),
                "mean_successful_steps": float(s["num_successful"].mean()),
                "iterations_histogram": {int(k): int(v) for k, v in zip(*np.unique(s["num_iterations"], return_counts=True))},
                "pose_gather": (("avm_gather_states (library, raw rccl.h; checked against torch.distributed's all_gather before the timed region)" if use_lib_gather and gather_checked else "avm_gather_states (library, raw rccl.h)" if use_lib_gather else ("torch.distributed all_gather through the host (gloo; ranks may share a device: "
                                "NOT a scaling measurement)" if gloo else "torch.distributed all_gather")) if world > 1 else "none (1 GPU)"),
                "per_rank_window_solve_kernel_ms": per_rank_solve_ms,
                "per_rank_gather_ms": per_rank_gather_ms,
                "launch": ("self-launched (bench.py spawned its ranks)" if os.environ.get("AVM_BENCH_SELF_LAUNCHED") else
                           ("external launcher (torch.distributed.run)" if world > 1 else "single process")),
                "input_generation_s": t_gen,
                "solve_form": solve_form + (" (two 256-thread workgroups per CU, window_solve_tp.o)" if solve_form == "throughput" else
                                            " (one 512-thread workgroup per CU)"),
                "marginalize_form": marg_form + (" (marginalize_tp_kernel: two 256-thread workgroups per CU)" if marg_form == "throughput" else
                                                 " (marginalize_kernel: one 512-thread workgroup per CU)"),
            },
            "roofline": {
                "bound": "mfma",
                "achieved": achieved,
                "peak": FP64_PEAK_TFLOPS,
                "unit": "TFLOP/s",
                "frac": achieved / FP64_PEAK_TFLOPS,
                "traffic": traffic,
                "traffic_source": traffic_src,
                "mfma_util": mfma_util,          # rocprof: MFMA pipe busy / SIMD-cycles (FP64 MFMA and FP64 VALU share the pipe on gfx950)
                "fabric_GBs": fabric_gbs,        # rocprof: L2 <-> fabric bytes per second (Infinity Cache hits included), peak ~8 TB/s HBM
                "wait_any_frac": wait_any,       # rocprof: SQ_WAIT_ANY / SQ_WAVE_CYCLES
                "kernel": solve_kernel,
                "kernel_ms": k_ms,
                "flops_per_launch": flops,
                "peak_measured": peak_meas,
                "hbm_secondary": {"algorithmic_bytes_per_launch": alg_bytes, "achieved_GBs": alg_bytes / (k_ms * 1e-3) / 1e9,
                                  "peak_GBs": HBM_PEAK_GBS},
            },
            "kernel_ms": {k: float(np.mean(v)) for k, v in all_ms.items()},
            # every kernel of the step against the same FP64 roofline; "furthest_below_roofline" names the one to work on next
            "kernel_rooflines": kernels,
            "furthest_below_roofline": furthest,
            # how far "parity" is pinned: the reference ships no tests / vectors and cannot be built here
            "parity_pin": "unpinned at the Ceres / Eigen boundary (no reference vectors exist, the reference does not build here): the oracle is pinned by "
                          "builder-written numpy restatements (tests/golden/) whose 50-digit runs (mpmath) and the oracle's binary128 build agree to 1e-25 over whole solves "
                          "(tests/test_solve_trace_mp.py) and to the rounding of the arbiter's FP64 output on the marginalization (test_marg_mp.py) and the selection "
                          "(test_fsel_mp.py); the 1-NN depth by the reference's own vendored nanoflann (tests/golden/nanoflann_nn.npz)",
        }

    # ---- sub-records the headline line does not carry: ragged tracks, one-window latency
    if extras and rank == 0:
        def timed_record(E_, win_, slots_, n_warm=3, n_timed=10):
            """A robust sub-record of a batch: n_warm untimed steps, then n_timed steps timed ONE BY ONE (a synchronization on
            both sides of each): median / min / max wall time, the per-step window_solve list, device allocations inside the
            timed region (none expected), and how the marginalization's square roots were taken."""
            keep = {k: win_.a[k].clone() for k in ("pose", "speedbias", "ex_pose", "inv_depth")}
            for opt_k in ("td", "relo_pose"):
                if opt_k in win_.a and win_.a[opt_k] is not None and hasattr(win_.a[opt_k], "clone"):
                    keep[opt_k] = win_.a[opt_k].clone()
            ms_k = {k: [] for k in ("preint", "window_solve", "marginalize", "prior_eig")}
            walls, ss_ = [], None

            def one():
                for k, v in keep.items():
                    win_.a[k].copy_(v)
                return E_.optimization(win_, want_summary=True, prior_out=slots_)

            for _ in range(n_warm):
                one()
            torch.cuda.synchronize()
            c0 = ctx.counters() if hasattr(ctx, "counters") else None
            for _ in range(n_timed):
                torch.cuda.synchronize()
                t_ = time.perf_counter()
                ss_ = one()
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t_)
                for k in ms_k:
                    ms_k[k].append(ctx.kernel_ms(k))
            c1 = ctx.counters() if hasattr(ctx, "counters") else None
            med = statistics.median(walls)
            rec = {"value": win_.n_windows / med, "unit": "solves/s", "ms_per_step": med * 1e3, "ms_per_step_min": min(walls) * 1e3,
                   "ms_per_step_max": max(walls) * 1e3, "steps": n_timed, "warmup": n_warm,
                   "kernel_ms": {k: float(statistics.median(v)) for k, v in ms_k.items()},
                   "window_solve_ms_per_step": [round(float(x), 4) for x in ms_k["window_solve"]],
                   "mean_iterations": float(buffers.summary_to_numpy(ss_)["num_iterations"].mean())}
            if c0 is not None:
                rec["allocations_inside_timed_region"] = c1["allocations"] - c0["allocations"]
                rec["solve_form"] = c1["solve_form"]
                if c1["prior_windows"]:
                    rec["prior_square_roots"] = {"one_wavefront_kernel": c1["prior_one_wavefront"], "pivoted_path": c1["prior_pivoted_path"]}
            return rec

        if sparse_base is not None:
            sh = synth.tile_windows(sparse_base, W)
            sw = sh.to_device(dev)
            rec = timed_record(E, sw, prior_slots)
            rec["workload"] = (f"{W} windows, 150 features with ragged tracks (start ~ U{{0..7}}, length ~ U{{2..}}), "
                               f"{float((sh.a['feat_nobs'] - 1).clip(min=0).sum(1).mean()):.0f} projection factors per window; "
                               f"{sparse_base.n_windows} distinct windows tiled")
            result["sparse_tracks"] = rec
            del sw
        if marg and W >= 1024:
            # the branch estimator.cpp:924-990 (MARGIN_SECOND_NEW) and the extended problem (estimator.cpp:672-688, 732-747, 760-792:
            # ex_pose and td as variables, a relocalization frame) on a quarter batch each: timed, not part of `value`
            o_sn = abi.default_options()
            o_sn.marginalization_flag = abi.MARGIN_SECOND_NEW
            qb = host.slice(0, W // 4).copy().to_device(dev)
            slots_q = buffers.PriorOutArrays.alloc(W // 4, qb.dims["max_prior"], qb.dims["max_pblk"], dev)
            rec = timed_record(est_m.Estimator(ctx=ctx, options=o_sn), qb, slots_q, n_warm=2, n_timed=5)
            rec["workload"] = f"{W // 4} of the headline windows, marginalization_flag = MARGIN_SECOND_NEW"
            result["margin_second_new"] = rec
            try:
                xh = synth.make_windows_parallel(min(W // 4, 256), first_id=rank * W, tracks="dense", procs=1, td_true=0.004, relo=True)
                xw = synth.tile_windows(xh, W // 4).to_device(dev)
                o_x = abi.default_options()
                o_x.estimate_extrinsic, o_x.estimate_td = 1, 1
                slots_x = buffers.PriorOutArrays.alloc(W // 4, xw.dims["max_prior"], xw.dims["max_pblk"], dev)
                rec = timed_record(est_m.Estimator(ctx=ctx, options=o_x), xw, slots_x, n_warm=2, n_timed=5)
                rec["workload"] = (f"{W // 4} dense windows with estimate_extrinsic = estimate_td = 1 and a relocalization frame: the -DAVM_X build of "
                                   "the solve kernel (178 x 178 reduced system, always the latency form)")
                # same FLOP model with the wider dense block: per linear solve 79 x 80 x F + 178^3 / 3
                result["extended_problem"] = rec
            except Exception as e:  # (a generator without the optional members: say so instead of failing the bench)
                result["extended_problem"] = {"unavailable": f"{type(e).__name__}: {e}"}
            del qb
        # one window per call, device-resident: the reference's own use (one optimization() per image)
        one = host.slice(0, 1).copy().to_device(dev)
        one0 = {k: one.a[k].clone() for k in ("pose", "speedbias", "ex_pose", "inv_depth")}
        po1 = buffers.PriorOutArrays.alloc(1, one.dims["max_prior"], one.dims["max_pblk"], dev) if marg else None
        lat = []
        for k in range(12):
            for kk, v in one0.items():
                one.a[kk].copy_(v)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            E.optimization(one, want_summary=False, prior_out=po1)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t1)
        result["latency_single_window_ms"] = {"value": statistics.median(lat[2:]) * 1e3, "what": "wall time of one avm_window_solve_batch call on one "
                                              "dense window (pre-integration, solve, marginalization, prior), device-resident buffers, median of 10",
                                              "kernel_ms": {k: ctx.kernel_ms(k) for k in ("preint", "window_solve", "marginalize", "prior_eig")}}
        if rank == 0 and not args.no_host_latency:
            try:
                result["latency_host_call_ms"] = host_call_latency(abi, synth)
            except Exception as e:  # (the hooks are test infrastructure: say so instead of failing the bench)
                result["latency_host_call_ms"] = {"unavailable": f"{type(e).__name__}: {e}"}

    # ---- feature selector: ms/frame (batch throughput), single-frame latency, FLOP/s of the scoring loop
    fsel_host = None
    if args.full and not args.no_fsel:
        FS = fs_m.FeatureSelector(ctx=ctx)
        P = args.fsel_problems
        fsel_host = synth.make_fsel(P, first_id=rank * P)
        fp = fsel_host.to_device(dev)
        f1 = synth.make_fsel(1, first_id=rank * P).to_device(dev)
        out_b = FS.select_batch(fp)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        reps = 3
        fsel_ms = []
        for _ in range(reps):
            FS.select_batch(fp)
            fsel_ms.append(ctx.kernel_ms("fsel_select"))
        torch.cuda.synchronize()
        tb = (time.perf_counter() - t1) / reps
        FS.select_batch(f1)
        t1 = time.perf_counter()
        for _ in range(reps):
            FS.select_batch(f1)
        torch.cuda.synchronize()
        tl = (time.perf_counter() - t1) / reps
        if rank == 0:
            # FLOPs of the scoring loop after the exact hoist: every round scores every live candidate with a
            # T x T (T = 3 H) Cholesky: T^3/3 + 2 T^2 FLOP per evaluation (forming C + p Delta, the factorization, log diag)
            _, _, valid = FS.information(fsel_host)
            nsel = out_b.to_host().a["n_selected"].astype(np.int64)
            nvalid = (valid != 0).sum(1).astype(np.int64)
            evals = float(sum(int(nv) * int(k) - int(k) * (int(k) - 1) // 2 for nv, k in zip(nvalid, nsel)))
            T = 3.0 * fsel_host.dims["horizon"]
            fl = evals * (T**3 / 3.0 + 2.0 * T * T)
            k_ms_f = float(np.mean(fsel_ms))
            result["feature_select"] = {
                "workload": "500 candidates -> 150 selected, horizon 10 (BASELINE.json configs[2])",
                "ms_per_frame_batched": tb / P * 1e3,
                "batch": P,
                "ms_per_frame_single": tl * 1e3,
                "roofline": {
                    "bound": "mfma", "unit": "TFLOP/s", "peak": FP64_PEAK_TFLOPS, "achieved": fl / (k_ms_f * 1e-3) / 1e12,
                    "frac": fl / (k_ms_f * 1e-3) / 1e12 / FP64_PEAK_TFLOPS, "kernel": "fsel_setup + fsel_frame_kernel (eight teams, one per XCD, take the frames from a queue), HIP events around the whole select",
                    "kernel_ms": k_ms_f, "flops_per_launch": fl, "candidate_evaluations": evals,
                    "reference_flops_unhoisted": evals * ((9.0 * (fsel_host.dims["horizon"] + 1)) ** 3 / 3.0),
                },
                "fallback_stats": ctx.fsel_fallback_stats(),
            }
            if extras:
                # the reference's compiled HORIZON (utility/state_defs.h:8): 13
                f13 = synth.make_fsel(P, first_id=rank * P, horizon=13).to_device(dev)
                f13_1 = synth.make_fsel(1, first_id=rank * P, horizon=13).to_device(dev)
                FS.select_batch(f13)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(reps):
                    FS.select_batch(f13)
                torch.cuda.synchronize()
                tb13 = (time.perf_counter() - t1) / reps
                FS.select_batch(f13_1)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(reps):
                    FS.select_batch(f13_1)
                torch.cuda.synchronize()
                tl13 = (time.perf_counter() - t1) / reps
                # larger batches (eight GPUs' worth of frames on one): from 33 frames on a batch takes the SOLO form of the selector on its own (one
                # workgroup per frame, lazy evaluation: csrc/fsel.hip, fsel_solo_kernel); the teams' time for the same batch is measured beside it
                big_b, big_form, big_teams, big_evals, big_kms = {}, {}, {}, {}, {}
                for Pb in (64, 128, 256, 512, 1024):  # (512 / 1024: two and four frames per CU's worth - where the solo form saturates: VERDICT r5 item 4)
                    fb = synth.make_fsel(min(Pb, 64), first_id=rank * P)
                    if Pb > 64:  # (tiled: the generator is the slow part)
                        fb = type(fb)(dict(fb.dims, n_problems=Pb), {k: np.ascontiguousarray(v[np.arange(Pb) % 64]) for k, v in fb.a.items()}, fb.scalars)
                    fbd = fb.to_device(dev)
                    for forced, store in ((None, big_b), ("0", big_teams)):
                        if forced is not None and Pb > 256:
                            continue
                        if forced is None:
                            os.environ.pop("AVM_FSEL_SOLO", None)
                        else:
                            os.environ["AVM_FSEL_SOLO"] = forced
                        FS.select_batch(fbd)
                        torch.cuda.synchronize()
                        if forced is None:
                            big_form[str(Pb)] = ctx.last_fsel_form()
                        t1 = time.perf_counter()
                        for _ in range(2):
                            FS.select_batch(fbd)
                        torch.cuda.synchronize()
                        store[str(Pb)] = (time.perf_counter() - t1) / 2 / Pb * 1e3
                        if forced is None:
                            big_evals[str(Pb)], big_kms[str(Pb)] = ctx.last_fsel_evaluations(), ctx.kernel_ms("fsel_select")
                    os.environ.pop("AVM_FSEL_SOLO", None)
                    del fbd
                result["feature_select"]["ms_per_frame_by_batch"] = big_b
                if big_form.get("256") == "solo" and big_evals.get("256", -1) > 0:
                    # the solo form (one workgroup per frame, lazy evaluation) priced on the evaluations it EXECUTES - counted on the device
                    # (fsel_solo_kernel adds every frame's scored candidates to a counter) - not on the hoisted full evaluation it
                    # proves unnecessary: T^3/3 + 2 T^2 FLOP each, HIP events around the whole select (setup + tree + solo kernel)
                    ev_s, k_s = float(big_evals["256"]), float(big_kms["256"])
                    result["feature_select"]["roofline_solo"] = {
                        "bound": "mfma", "unit": "TFLOP/s", "peak": FP64_PEAK_TFLOPS, "batch": 256, "kernel": "fsel_kdtree + fsel_setup + fsel_solo_kernel, HIP events around the whole select",
                        "kernel_ms": k_s, "candidate_evaluations_executed": ev_s, "candidate_evaluations_full_greedy": evals / P * 256,
                        "executed_fraction": ev_s / (evals / P * 256), "flops_per_launch": ev_s * (T**3 / 3.0 + 2.0 * T * T),
                        "achieved": ev_s * (T**3 / 3.0 + 2.0 * T * T) / (k_s * 1e-3) / 1e12,
                        "frac": ev_s * (T**3 / 3.0 + 2.0 * T * T) / (k_s * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                        "frac_if_priced_on_the_full_greedy": (evals / P * 256) * (T**3 / 3.0 + 2.0 * T * T) / (k_s * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                    }
                result["feature_select"]["form_by_batch"] = big_form
                result["feature_select"]["ms_per_frame_by_batch_teams_forced"] = big_teams
                # the pipelined deployment: single-frame selects while ANOTHER ctx runs the 4096-window solve on the same device
                import threading

                ctx2 = lib_m.Context(local_rank)
                E2c = est_m.Estimator(ctx=ctx2, options=opt)
                stop_ev, n_solves = threading.Event(), [0]

                def _solver():
                    pr2 = buffers.PriorOutArrays.alloc(W, win.dims["max_prior"], win.dims["max_pblk"], dev) if marg else None
                    while not stop_ev.is_set():
                        E2c.optimization(win, want_summary=False, prior_out=pr2)
                        n_solves[0] += 1

                th = threading.Thread(target=_solver)
                th.start()
                lat_c = []
                try:
                    while n_solves[0] < 1:
                        time.sleep(0.005)
                    for _ in range(12):
                        t1 = time.perf_counter()
                        FS.select_batch(f1)
                        torch.cuda.synchronize()
                        lat_c.append(time.perf_counter() - t1)
                finally:
                    stop_ev.set()
                    th.join(timeout=120)
                result["feature_select"]["ms_per_frame_single_beside_a_solve"] = {
                    "median": statistics.median(lat_c) * 1e3, "min": min(lat_c) * 1e3, "max": max(lat_c) * 1e3,
                    "what": f"12 single-frame selects while a second ctx loops the {W}-window solve on the same device ({n_solves[0]} solves meanwhile): "
                            "the select queues behind the solve's kernels (they fill every CU)", "fallback_stats": ctx.fsel_fallback_stats()}
                result["feature_select"]["horizon_13"] = {"workload": "500 candidates -> 150 selected, HORIZON 13 (the reference's compiled value, utility/state_defs.h:8)",
                                                          "ms_per_frame_batched": tb13 / P * 1e3, "batch": P, "ms_per_frame_single": tl13 * 1e3}
                # ... and a large batch of it (the solo form; the teams' time for the same batch beside it)
                f13b = synth.make_fsel(64, first_id=rank * P, horizon=13)
                f13b = type(f13b)(dict(f13b.dims, n_problems=256), {k: np.ascontiguousarray(v[np.arange(256) % 64]) for k, v in f13b.a.items()}, f13b.scalars).to_device(dev)
                for forced, key in ((None, "ms_per_frame_batch_256"), ("0", "ms_per_frame_batch_256_teams_forced")):
                    if forced is None:
                        os.environ.pop("AVM_FSEL_SOLO", None)
                    else:
                        os.environ["AVM_FSEL_SOLO"] = forced
                    FS.select_batch(f13b)
                    torch.cuda.synchronize()
                    if forced is None:
                        result["feature_select"]["horizon_13"]["form_batch_256"] = ctx.last_fsel_form()
                    t1 = time.perf_counter()
                    FS.select_batch(f13b)
                    torch.cuda.synchronize()
                    result["feature_select"]["horizon_13"][key] = (time.perf_counter() - t1) / 256 * 1e3
                os.environ.pop("AVM_FSEL_SOLO", None)
                del f13b

    # ---- CPU baseline (oracle = port of the reference algorithm), rank 0, N=1 only
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import oracle_py

        build = native_oracle()
        o2 = abi.default_options()
        o2.marginalization_flag = opt.marginalization_flag

        def solve_sample(n, threads):
            smp = host.slice(0, n).copy()
            po = buffers.PriorOutArrays.alloc(n) if o2.marginalization_flag != abi.MARGIN_NONE else None
            sm = buffers.summary_alloc(n)
            return lambda: oracle_py.window_solve(o2, smp.copy(), po, sm, n_threads=threads)

        n1 = min(W, 6)
        r1, p1 = median_rate(solve_sample(n1, 1), n1, passes=5, budget_s=6.0)
        nall = min(W, max(2 * ncpu, 16))
        rall, pall = median_rate(solve_sample(nall, ncpu), nall, passes=5, budget_s=12.0)
        # second leg, "port_blocked": the same port with its Schur update / Cholesky / forward substitution in a form the compiler
        # vectorises (oracle/linalg.hpp, bit-for-bit the same operations in the same order; asserted against the literal loops in the CPU tier)
        blocked = None
        if hasattr(oracle_py, "set_fast_linalg"):
            oracle_py.set_fast_linalg(True)
            try:
                rb1, _ = median_rate(solve_sample(n1, 1), n1, passes=5, budget_s=6.0)
                rball, pball = median_rate(solve_sample(nall, ncpu), nall, passes=5, budget_s=12.0)
            finally:
                oracle_py.set_fast_linalg(False)
            blocked = {"value": rball, "unit": "solves/s", "cores": ncpu, "kind": "port_blocked", "value_1_core": rb1,
                       "sample": f"as the literal port ({nall} windows per pass on {ncpu} threads, median of {pball} passes)",
                       "socket_extrapolated": {"value": rb1 * 64, "unit": "solves/s", "cores": 64, "gpu_over_cpu_socket": value / (rb1 * 64)}}
        scaling = {}
        for th in sorted({max(1, ncpu // 4), max(1, ncpu // 2)} - {1, ncpu}):
            nn = min(W, max(2 * th, 16))
            scaling[str(th)] = median_rate(solve_sample(nn, th), nn, passes=3, budget_s=5.0)[0]
        result["cpu_baseline"] = {
            "value": rall,
            "unit": "solves/s",
            "cores": ncpu,
            "kind": "port",
            "sample": f"{nall} of the same windows per pass, one single-threaded solve per host thread ({ncpu} threads = every CPU this process "
                      f"may run on), median of {pall} passes; 1 thread: {n1} windows per pass, median of {p1} passes",
            "value_1_core": r1,
            "threads_scaling": scaling,
            "build": build,
            "cpu": cpu_info,
            # what a whole socket of this host would do, ASSUMING the linear thread scaling measured above continues
            # (one independent single-threaded solve per core, no shared state): an extrapolation, not a measurement
            "socket_extrapolated": {"value": r1 * 64, "unit": "solves/s", "cores": 64,
                                    "how": f"value_1_core x 64 physical cores of one {cpu_info['model']} socket; measured up to {ncpu} threads",
                                    "gpu_over_cpu_socket": value / (r1 * 64)},
        }
        if blocked is not None:
            result["cpu_baseline"]["port_blocked"] = blocked
            # the ratio the >= 50x target is quoted against: the FASTER of the two ports, a whole socket (extrapolated from one core)
            best1 = max(r1, blocked["value_1_core"])
            result["gpu_over_cpu_socket"] = {"value": value / (best1 * 64), "against": "port_blocked" if blocked["value_1_core"] >= r1 else "port",
                                             "how": "value / (the faster port's 1-core rate x 64 cores): an extrapolation, stated as one"}
        result["gpu_over_cpu"] = value / rall
        result["gpu_over_cpu_1_core"] = value / r1
        if fsel_host is not None:
            nf = min(fsel_host.n_problems, 2)
            f_smp = synth.make_fsel(nf, first_id=0)
            oo = buffers.FselOutArrays.alloc(nf, 150)
            rf1, pf1 = median_rate(lambda: oracle_py.fsel_select(f_smp, oo, n_threads=1), nf, passes=3, budget_s=8.0)
            result["feature_select"]["cpu_baseline"] = {
                "value": 1e3 / rf1, "unit": "ms/frame", "cores": 1, "kind": "port",
                "sample": f"{nf} frames of the same workload per pass on one host thread (the reference selects on one thread), median of {pf1} passes; "
                          "the oracle follows feature_selector.cpp:613-728 literally (dense 9(H+1) x 9(H+1) Cholesky per evaluation, lazy upper-bound break)",
                "build": build,
            }
            result["feature_select"]["gpu_over_cpu_1_core_batched"] = (1e3 / rf1) / result["feature_select"]["ms_per_frame_batched"]

    if rank == 0:
        # The numbers a reader of a truncated line needs, once more, compact and LAST (a log that keeps the tail of stdout keeps this):
        def _g(d, *path):
            for k in path:
                d = d.get(k) if isinstance(d, dict) else None
                if d is None:
                    return None
            return round(d, 4) if isinstance(d, float) else d
        fsr = result.get("feature_select", {})
        result["summary"] = {
            "value": _g(result, "value"), "ms_per_step": _g(result, "ms_per_step"), "kernel_ms": {k: round(v, 3) for k, v in result.get("kernel_ms", {}).items()},
            "frac": {k: _g(v, "frac") for k, v in result.get("kernel_rooflines", {}).items()},
            "sparse_tracks": _g(result, "sparse_tracks", "value"), "margin_second_new": _g(result, "margin_second_new", "value"),
            "extended_problem": _g(result, "extended_problem", "value"), "latency_single_window_ms": _g(result, "latency_single_window_ms", "value"),
            "latency_host_call_ms": {"optimization": _g(result, "latency_host_call_ms", "optimization", "value"), "select": _g(result, "latency_host_call_ms", "select", "value")},
            "fsel_ms_per_frame": {"batch16": _g(fsr, "ms_per_frame_batched"), "single": _g(fsr, "ms_per_frame_single"), "by_batch": fsr.get("ms_per_frame_by_batch"),
                                  "h13_batch16": _g(fsr, "horizon_13", "ms_per_frame_batched"), "h13_single": _g(fsr, "horizon_13", "ms_per_frame_single"),
                                  "h13_batch256": _g(fsr, "horizon_13", "ms_per_frame_batch_256")},
            "fsel_frac": {"teams16": _g(fsr, "roofline", "frac"), "solo256_executed": _g(fsr, "roofline_solo", "frac"),
                          "solo256_executed_fraction_of_full_greedy": _g(fsr, "roofline_solo", "executed_fraction")},
            "cpu": {"solves_per_s": _g(result, "cpu_baseline", "value"), "cores": _g(result, "cpu_baseline", "cores"), "one_core": _g(result, "cpu_baseline", "value_1_core"),
                    "fsel_ms_per_frame_1_core": _g(fsr, "cpu_baseline", "value")},
        }
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
