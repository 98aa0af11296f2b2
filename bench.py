#!/usr/bin/env python3
"""bench.py -- samples/s of regressor build + TSQR base-parameter solve on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path over this rank's resident batch of synthetic (q, qd, qdd):
K1 regressor assembly (W materialised in the reference layout, column norms fused) -> elimination ->
K3 Householder TSQR over the kept columns + tau -> host tail (rank decision, regrouping, beta, strings,
phi) -> [N>1: RCCL all-reduce of column norms + all-gather of R factors].  Inputs are resident in HBM
before the timed region.  Default workload = BASELINE.json configs[1] (UR10 6-DoF, 1e6 samples per GPU: weak scaling).  --config cfg3|cfg4|cfg5 runs
the other BASELINE configs (TIAGo 1e6, TALOS 4e6, human 1e7 streamed), by default with STRONG scaling: the config's total
sample count is sharded over the GPUs (north_star: >= 6x at 8 GPUs on the sharded configs).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfgK] [--scaling weak|strong] [--samples S] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6   # MI355X datasheet: fp64 vector == fp64 matrix (v_mfma_f64_16x16x4) peak
HBM_PEAK_GBS = 8000.0     # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)


def cpu_quota():
    """CPUs this process may actually use: the cgroup quota if there is one (the GPU boxes show 256 logical CPUs under a
    quota of 16), else None.  Threads beyond the quota do not add throughput, they get the whole process frozen until
    the next accounting period."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:  # cgroup v2
            quota, period = f.read().split()
        if quota != "max":
            return float(quota) / float(period)
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:  # cgroup v1
            quota = float(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            period = float(f.read())
        if quota > 0:
            return quota / period
    except Exception:
        pass
    return None


def _baseline_threads():
    """Thread cap for the CPU baseline legs: the quota when there is one (so the baseline is not throttled)."""
    quota = cpu_quota()
    if quota is None:
        return None
    n = max(1, int(quota))
    os.environ.setdefault("OMP_NUM_THREADS", str(n))  # the OpenMP regressor of oracle/ (read when its runtime starts)
    return n


class _Threads:
    def __init__(self, n):
        self.n, self.ctx = n, None

    def __enter__(self):
        if self.n:
            try:
                from threadpoolctl import threadpool_limits
                self.ctx = threadpool_limits(limits=self.n)
            except Exception:
                self.ctx = None
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.restore_original_limits()
        return False


def _cpu_inputs(robot, cfg, seed, n_cpu):
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    rng = np.random.default_rng(seed)
    if cfg == "cfg2":
        q, v, a = (rng.uniform(-6, 6, (n_cpu, 6)) for _ in range(3))
    else:
        q, v, a = sample_inputs(robot.model, n_cpu, rng, 1.5, 2, 5)
    return q, v, a, rng.standard_normal(robot.model.nv * n_cpu)


def cpu_baseline(robot, cfg, param, seed, n_cpu, n_config):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    cap = _baseline_threads()
    import cpu_baseline as cb  # oracle: measured here as the reported baseline, never shipped

    flat = robot.model.to_flat()
    q, v, a, tau = _cpu_inputs(robot, cfg, seed, n_cpu)
    with _Threads(cap):
        t0 = time.perf_counter()
        _, stages = cb.faithful_pass(flat, q, v, a, tau, friction=bool(param["has_friction"]),
                                     actuator_inertia=bool(param["has_actuator_inertia"]),
                                     offset=bool(param["has_joint_offset"]))
        dt = time.perf_counter() - t0
        try:
            from threadpoolctl import threadpool_info
            blas = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
        except Exception:
            blas = os.cpu_count()
    nv = robot.model.nv
    note = ""
    if cfg != "cfg2":
        # where the faithful path cannot allocate the config's size (W and W_mod: 2 x 64.5 GB for TIAGo at
        # 1e6 samples, plus Q of the two QRs), it is timed at the largest N that fits and the extrapolation is stated
        note = ("; measured at N = %d because the reference structure needs 2 x %.1f GB for W / W_mod (+ explicit Q) at "
                "the config's %d samples -- every stage is linear in N, so the rate carries over" % (
                    n_cpu, 8.0 * nv * n_config * 14 * nv / 1e9, n_config))
    return {
        "value": n_cpu / dt, "unit": "samples/s", "cores": int(blas), "cpu_quota_cpus": cpu_quota(), "kind": "port",
        "sample": "%d of the %d %s samples, faithful reference structure (python per-sample loop around the C "
                  "regressor of oracle/, numpy scatter+permutation, np.diag(W.T@W), np.delete, 2x np.linalg.qr, "
                  "pinv); host has %d logical cpus, BLAS threads %d; stage seconds %s%s" % (
                      n_cpu, n_config, robot.model.name, os.cpu_count(), blas,
                      {k: round(x, 2) for k, x in stages.items()}, note),
    }


def cpu_baseline_fast(robot, cfg, param, seed, n_cpu, n_config):
    """The same pass with the host used well (OpenMP regressor in C, QR without Q): SURVEY 8(d) "fair-fast"."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import cpu_baseline as cb

    flat = robot.model.to_flat()
    q, v, a, tau = _cpu_inputs(robot, cfg, seed, n_cpu)
    flags = (1 if param["has_friction"] else 0) | (2 if param["has_actuator_inertia"] else 0) | (4 if param["has_joint_offset"] else 0)
    nv = robot.model.nv
    cap = _baseline_threads()
    with _Threads(cap):
        cb.fast_pass(flat, q[:2000], v[:2000], a[:2000], tau[:nv * 2000], flags=flags)  # thread pools up
        t0 = time.perf_counter()
        _, stages = cb.fast_pass(flat, q, v, a, tau, flags=flags)
        dt = time.perf_counter() - t0
    return {"value": n_cpu / dt, "unit": "samples/s", "cores": cap or os.cpu_count(), "cpu_quota_cpus": cpu_quota(),
            "kind": "port",
            "sample": "%d of the %d %s samples, fair-fast structure (one OpenMP C call for the batch regressor, einsum "
                      "column norms, np.linalg.qr(mode='r') of [W_e tau], regrouped QR of the triangle, triangular solves); "
                      "host has %d logical cpus, threads capped at the cgroup quota when there is one; stage seconds %s" % (
                          n_cpu, n_config, robot.model.name, os.cpu_count(), {k: round(x, 2) for k, x in stages.items()})}


CONFIGS = {  # BASELINE.json configs[1..4]: (golden fixture, model, samples in the config, chunk for the streamed pass)
    "cfg2": ("cfg2_ur10", "ur10", 1_000_000, None),
    "cfg3": ("cfg3_tiago", "tiago", 1_000_000, None),
    "cfg4": ("cfg4_talos", "talos", 4_000_000, None),
    # cfg5: W RESIDENT since round 5 -- the link-compact layout (21 massless links of the human model have no columns: 146 GB
    # for 6e7 rows instead of 307 GB) fits HBM in one piece: 122 ms against 131 ms streamed in chunks of 2.5e6 samples
    # (--chunk-samples 2500000; 151 ms in round 4 with 67 GB link-padded chunks)
    "cfg5": ("cfg5_human", "human", 10_000_000, None),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS),
                    help="cfg2 (default) = the workload the metric is quoted on; cfg3-5 = the other BASELINE configs")
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"],
                    help="weak: --samples per GPU (default for cfg2); strong: the config's total sharded over the GPUs "
                         "(default for cfg3-5)")
    ap.add_argument("--samples", type=int, default=None, help="samples per GPU (weak) / in total (strong)")
    ap.add_argument("--chunk-samples", type=int, default=None,
                    help="cfg5: stream the samples in chunks of this size (figh_regressor_tsqr) instead of keeping W resident")
    ap.add_argument("--cpu-samples", type=int, default=None,
                    help="samples of the CPU baseline legs (default: 300000 for cfg2, 20000 for cfg3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--exchange", default="rccl", choices=["rccl", "torch", "host"],
                    help="rccl: device buffers over RCCL / xGMI; torch / host: host-staged through the control plane")
    ap.add_argument("--rendezvous", default="socket", choices=["torch", "socket"],
                    help="control plane of a multi-rank run (RCCL id exchange, barriers, max over ranks): torch.distributed "
                         "(gloo) or figaroh_plus_amd.dist.SocketGroup (standard library only: no PyTorch in the process)")
    ap.add_argument("--placement-trials", type=int, default=1,
                    help="set-up (untimed): candidate allocations of W among which the one K1 writes fastest is kept "
                         "(IdentificationPipeline.placement_trials; 1 = take the first, the default since round 4: the fused "
                         "launch writes W at half the rate the stand-alone regressor kernel needs and does not depend on it)")
    ap.add_argument("--structural-zeros", default="every-pass", choices=["every-pass", "once"],
                    help="once = opt-in variant for the joint-torque regressor of a tree (cfg3): W is zero-filled at set-up "
                         "and the regressor kernel leaves its structural zeros alone (FIGH_FLAG_ZEROS_PRESENT); every entry "
                         "that depends on the inputs is still written in every pass.  Reported in config.structural_zeros; "
                         "the default re-creates every byte of W in every pass")
    ap.add_argument("--w-layout", default="auto", choices=["auto", "dense", "block-compact"],
                    help="how W is kept in HBM.  dense = the reference's rows (link-padded for trees).  block-compact (trees "
                         "in joint-torque mode, cfg3) = row block j as its own N x 16 |subtree_j| matrix: only the window of a "
                         "row that can be non-zero is stored, written and read, every stored byte in every pass "
                         "(FIGH_FLAG_COMPACT_BLOCKS).  auto = block-compact where it applies; config.w_layout says which")
    ap.add_argument("--active-joints", action="store_true",
                    help="cfg3: only the row blocks of the eight joints that carry measurements in the TIAGo script (torso_lift, "
                         "arm_1..7: examples/tiago/identification.py:406-424) are stored and factored "
                         "(IdentificationPipeline(row_blocks=act_idxv)); the elimination still uses the norms of all 24 blocks")
    ap.add_argument("--no-wls", action="store_true",
                    help="cfg3: leave the weighted least squares (examples/staubli_TX40/identification.py:305-346) out of the "
                         "timed step (default: included, as BASELINE configs[2] says \"WLS solve\")")
    ap.add_argument("--no-null-pivots", action="store_true",
                    help="plain Householder column steps for the dependent columns too (figh_tsqr_null_pivot_tol = 0)")
    ap.add_argument("--no-fuse", action="store_true",
                    help="cfg2: K1 and the level-0 TSQR as two launches (W written, then read back) instead of the fused "
                         "launch figh_regressor_tsqr_fused (default: fused from the second pass on; config.fused says which)")
    ap.add_argument("--strong-config", default="cfg4", choices=["", "cfg3", "cfg4", "cfg5"],
                    help="after the headline workload, a fixed-total-size (strong-scaling) measurement of this sharded BASELINE "
                         "config on the same ranks, reported as `strong_scaling` in the same line (north_star: >= 6x strong "
                         "scaling at 8 GPUs); '' = leave it out")
    ap.add_argument("--strong-samples", type=int, default=None, help="total samples of that measurement (default: the config's)")
    ap.add_argument("--strong-steps", type=int, default=5)
    ap.add_argument("--host-wait", default=None, choices=["spin", "block"],
                    help="how the host waits for the GPU: spin (default for one GPU) or block = interrupt-driven (default "
                         "for several ranks on a node: spinning ranks can exhaust a container's CPU quota)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step of the headline workload returned (every "
                         "numeric entry of IdentificationPipeline.run's result) as DIR/<name>.npy in float64 (rank 0); the "
                         "inputs are seeded, so two builds run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # the shipped library has no run-time switches; FIGH_LIB_PATH would swap in another build (tools/ A/B runs only)
    stray = sorted(k for k in os.environ if k.startswith("FIGH_"))
    if stray:
        raise SystemExit("bench.py refuses to run with FIGH_* variables set: %s" % ", ".join(stray))

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: this process becomes one (it has not touched the GPU and never will) -- see spawn_ranks
        raise SystemExit(spawn_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher's WORLD_SIZE is %d" % (args.gpus, world))

    from figaroh_plus_amd import _lib
    from figaroh_plus_amd.dist import exchange_from_env, shard_range
    from figaroh_plus_amd.pipeline import IdentificationPipeline
    from figaroh_plus_amd.tools.randomdata import sample_inputs
    from figaroh_plus_amd.tools.robot import Robot

    lib = _lib.load()
    if _lib.device_count() == 0:
        raise SystemExit("bench.py needs a HIP device: libfigh has no CPU path")
    host_wait = args.host_wait or ("block" if world > 1 else "spin")
    _lib.check(lib.figh_host_wait_mode(1 if host_wait == "block" else 0))
    _lib.check(lib.figh_device_set(local_rank % _lib.device_count()))
    exchange, xinfo = exchange_from_env(args.exchange, rendezvous=args.rendezvous)
    group = getattr(exchange, "control", None)  # the control plane of the run (None for one rank)

    def barrier():
        _lib.synchronize()
        if world > 1:
            group.barrier()

    def measure(args, steps, warmup, with_cpu, dump_dir=None):
        """One BASELINE config measured on the ranks of this run: (line of rank 0 | None, structural result ok)."""
        fixture, model_name, n_config, chunk = CONFIGS[args.config]
        if args.chunk_samples and args.config == "cfg5":
            chunk = args.chunk_samples
        scaling = args.scaling or ("weak" if args.config == "cfg2" else "strong")
        with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
            meta = json.load(f)
        robot = Robot.from_flat(model_name)
        param = meta["param"]
        params_std = dict(zip(meta["names_std"], meta["phi_ref_raw"]))
        if scaling == "weak":
            N = args.samples or n_config          # per GPU
            n_total = N * world
        else:
            n_total = args.samples or n_config    # sharded: contiguous sample ranges (dist.shard_range)
            lo, hi = shard_range(n_total, rank, world)
            N = hi - lo
        rng = np.random.default_rng(20250410 + int(args.config[3]) + 1000 * rank)
        if args.config == "cfg2":  # examples/ur10/identification.py:71-81
            q, v, a = (rng.uniform(-6, 6, (N, 6)) for _ in range(3))
        else:
            q, v, a = sample_inputs(robot.model, N, rng, 1.5, 2, 5)
        row_blocks = None
        if args.active_joints:
            if args.config != "cfg3":
                raise SystemExit("--active-joints is the TIAGo script's variant (cfg3)")
            names = ["torso_lift_joint"] + ["arm_%d_joint" % k for k in range(1, 8)]
            row_blocks = [robot.model.joints[robot.model.getJointId(n)].idx_v for n in names]
        pipe = IdentificationPipeline(robot, param, params_std=params_std, coupling=meta["coupling"], exchange=exchange,
                                      row_blocks=row_blocks,
                                      chunk_samples=chunk, placement_trials=args.placement_trials,
                                      structural_zeros=args.structural_zeros,
                                      w_layout="dense" if args.w_layout == "dense" else "block-compact", fuse=not args.no_fuse,
                                      null_pivots=not args.no_null_pivots)
        # (the page-locked staging buffers of the bulk copies are allocated by the first large transfer: not part of the rate)
        _lib.DeviceArray.from_host(np.zeros(4 << 20)).free()
        _lib.synchronize()
        t_h2d = time.perf_counter()
        pipe.set_samples(q, v, a)
        _lib.synchronize()
        t_h2d = time.perf_counter() - t_h2d - 1e-3 * getattr(pipe, "repack_ms", 0.0)
        input_bytes = q.nbytes + v.nbytes + a.nbytes
        # ... and the copies alone, into a buffer that exists (set_samples above also allocates three device arrays)
        d_probe = _lib.DeviceArray((max(q.size, v.size),), np.float64)
        _lib.synchronize()
        t_copy = time.perf_counter()
        for arr in (q, v, a):
            _lib.check(lib.figh_memcpy_h2d(d_probe.ptr, arr.ctypes.data, arr.nbytes))
        _lib.synchronize()
        t_copy = time.perf_counter() - t_copy
        d_probe.free()
        phi_ref = np.array([float(x) for x in meta["phi_ref_raw"]])
        # cfg3 is quoted with a WLS solve (BASELINE configs[2]): measurement noise, or the per-joint variances are round-off
        pipe.set_tau_from_parameters(phi_ref, noise_std=0.05 if args.config in ("cfg2", "cfg3") else 0.0, seed=rank)
        wls = args.config == "cfg3" and not args.no_wls
        del q, v, a

        out = None
        # live HIP-event timing of the dominant kernels on the library stream (level 1: the event pair of K1 and of the TSQR
        # level 0 is stamped by their own dispatch packets, hipExtLaunchKernelGGL -- no extra packets in the queue), switched
        # on during warm-up already so that the event pool exists before the timed region
        _lib.profile_enable(True, level=1)
        for _ in range(warmup):
            out = pipe.run(wls=wls)
        _lib.profile_reset()
        barrier()
        step_times = []
        t0 = time.perf_counter()
        for _ in range(steps):
            ts = time.perf_counter()
            out = pipe.run(wls=wls)  # returns when its results are on the host: the per-step clock needs no extra synchronisation
            step_times.append(time.perf_counter() - ts)
        barrier()
        dt = time.perf_counter() - t0
        _lib.profile_enable(False)
        if dump_dir is not None and rank == 0:
            # (before the untimed passes below: they run the same pipeline again)
            dump_outputs(out, dump_dir)
        dt_rank = dt
        if world > 1:
            dt = max(group.all_gather_object(dt))

        # sanity: the step produced the reference's structural result (cfg3 at 1e6 samples: four dependent pivots grow past
        # TOL_QR like sqrt(N), LAPACK agrees -- DESIGN.md section 4 -- so only the eliminated columns are compared there)
        ok = out["idx_e"] == [int(x) for x in np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))["idx_e"]]
        if args.config != "cfg3":
            ok = ok and out["idx_base"] == meta_idx(meta) and out["params_base"] == meta["params_base"]
        elif world == 1 and N == 1_000_000 and not args.active_joints:
            # cfg3 at the BASELINE size: the index set a LAPACK Householder TSQR of the oracle's W keeps for THESE samples
            # (tests/golden/cfg3_tiago_large.json, oracle/pin_cfg3_large.py: 185 base parameters -- six pivots of the golden's
            # dependent columns have grown past TOL_QR like sqrt(N))
            with open(os.path.join(ROOT, "tests", "golden", "cfg3_tiago_large.json")) as f:
                pin = next(c for c in json.load(f)["cases"] if c["N"] == N and c["seed"] == 20250410 + 3)
            ok = ok and out["idx_base"] == pin["idx_base"]
        n_kept = len(out["params_r"])
        kern = {}
        k1_name = "regressor_chain" if args.config == "cfg2" else "regressor_tree"
        for name in (k1_name, "tsqr", "fused_chain_tsqr"):
            cnt, ms = _lib.profile_get(name)
            if cnt:
                kern[name] = {"launches": cnt, "avg_ms": ms / cnt}
        # FIRST pass: what a script that calls the identification functions once pays (examples/ur10/identification.py:71-83) --
        # the pipeline forgets everything it has learnt from earlier passes (kept-column set, counts, per-block lists; the HBM
        # buffers stay allocated) and runs one pass; median of five.  Collective-safe: every rank forgets and runs.
        first_times = []
        fused_before = pipe.fused_passes
        for _ in range(5):
            pipe.forget()
            barrier()
            ts = time.perf_counter()
            pipe.run(wls=wls)
            first_times.append(time.perf_counter() - ts)
        first_fused = pipe.fused_passes - fused_before
        # the small launches (merge levels, regrouped n x n factorisation, collectives) are timed in two extra,
        # untimed passes so that their event records do not sit in the timed region
        _lib.profile_enable(True, level=2)
        _lib.profile_reset()
        for _ in range(2):
            pipe.run(wls=wls)
        for name in ("triangle_residuals", "tsqr_tree", "tsqr_reduce", "select_columns", "rccl_allgather", "rccl_allreduce"):
            cnt, ms = _lib.profile_get(name)
            if cnt:
                kern[name] = {"launches_per_step": cnt / 2.0, "avg_ms": ms / cnt, "timed_region": False}
        _lib.profile_enable(False)
        transfers = {"h2d_inputs_ms": 1e3 * t_h2d, "h2d_inputs_GBps": input_bytes / t_h2d / 1e9, "timed_region": False,
                     "h2d_note": "set_samples: three device allocations + the copies; the copies alone: h2d_copy_*",
                     "h2d_copy_ms": 1e3 * t_copy, "h2d_copy_GBps": input_bytes / t_copy / 1e9,
                     # tree models: q, v, a re-laid per 64-sample tile once after the upload (figh_repack_samples), part of
                     # "device-resident q, v, a -> result" but not of the repeated pass (the copies stay resident)
                     "repack_inputs_ms": getattr(pipe, "repack_ms", 0.0)}
        if rank == 0 and pipe.W is not None and getattr(pipe, "_compact", None) is None and pipe.W.buf.size * 8 <= 8e9:
            # what the drop-in boundary pays when W itself is handed back to a NumPy caller (never part of `value`)
            from figaroh_plus_amd.device import host_empty
            _lib.synchronize()
            td = time.perf_counter()
            # (allocation included: a fresh huge-page-backed array per call, as GpuMatrix.numpy() / build_regressor_basic
            # return it; the resident buffer -- force-compact W is smaller than rows x ld)
            host_W = host_empty(pipe.W.buf.size)
            _lib.check(lib.figh_memcpy_d2h(host_W.ctypes.data, pipe.W.buf.ptr, host_W.nbytes))
            td = time.perf_counter() - td
            transfers.update({"d2h_W_ms": 1e3 * td, "d2h_W_GBps": host_W.nbytes / td / 1e9, "W_bytes": host_W.nbytes,
                              "d2h_path": "fresh huge-page-backed ndarray (device.host_empty) + staged 32 MB chunks, 8 copy "
                                          "threads (figh_memcpy_d2h)"})
            del host_W
            if args.config == "cfg2":
                # the whole drop-in call a FIGAROH script makes (regressor.py:20-194): host q, v, a in, host W out
                from figaroh_plus_amd.tools.regressor import build_regressor_basic
                rng2 = np.random.default_rng(1)
                q2, v2, a2 = (rng2.uniform(-6, 6, (N, 6)) for _ in range(3))
                build_regressor_basic(robot, q2[:1000], v2[:1000], a2[:1000], param)
                _lib.synchronize()
                td = time.perf_counter()
                W_host = build_regressor_basic(robot, q2, v2, a2, param)
                td = time.perf_counter() - td
                transfers.update({"drop_in_build_regressor_basic_ms": 1e3 * td,
                                  "drop_in_samples_per_s": N / td, "drop_in_W_shape": list(W_host.shape)})
                del W_host, q2, v2, a2
        m = robot.model
        rows_per_sample = m.nv if param["is_joint_torques"] else 6
        ncols = len(meta["names_std"])
        bytes_per_sample = 8 * (m.nq + 2 * m.nv) + 8 * rows_per_sample * ncols        # SURVEY 8(d), stage A
        flops_per_sample = 2 * rows_per_sample * (n_kept + 1) ** 2                    # SURVEY 8(d), stage B: 2 m n^2
        launches_per_step = {k: v["launches"] / float(steps) for k, v in kern.items() if "launches" in v}
        roof = {}
        if k1_name in kern:
            sec = kern[k1_name]["avg_ms"] * 1e-3 * launches_per_step[k1_name]  # (the streamed pass runs K1' twice per chunk)
            roof[k1_name] = {"bound": "hbm", "achieved": bytes_per_sample * N / sec / 1e9, "peak": HBM_PEAK_GBS,
                             "unit": "GB/s", "traffic": None, "algorithmic_bytes_per_sample": bytes_per_sample}
            if getattr(pipe, "_compact", None) is not None:
                # block-compact W: the kernel is asked to write the N x 16 |subtree_j| window of every row block, not the
                # reference's dense rows -- `achieved` / `frac` count the bytes this layout stores (every one of them is written
                # in every pass); the rate on the reference's dense bytes is kept beside them and is not a fraction of anything
                stored = 8 * (m.nq + 2 * m.nv) + 8 * float(pipe._compact[1].sum())
                roof[k1_name].update({"achieved": stored * N / sec / 1e9, "algorithmic_bytes_per_sample": stored,
                                      "dense_bytes_per_sample": bytes_per_sample,
                                      "dense_equivalent_GBps": bytes_per_sample * N / sec / 1e9})
            if getattr(pipe, "_link_pos", None) is not None or getattr(pipe, "_force_ld", 0):
                # link-compact / force-compact W: links without entries (massless bodies) have no columns, the force rows one
                # line per four links; same accounting as above
                stored = 8 * (m.nq + 2 * m.nv) + 8.0 * pipe.W.buf.size / pipe.N
                roof[k1_name].update({"achieved": stored * N / sec / 1e9, "algorithmic_bytes_per_sample": stored,
                                      "dense_bytes_per_sample": bytes_per_sample,
                                      "dense_equivalent_GBps": bytes_per_sample * N / sec / 1e9})
        if "fused_chain_tsqr" in kern:
            # one launch does stage A (the regressor, written to HBM) and stage B level 0 (the TSQR of the kept columns, out of
            # LDS): its time is bounded from below by max(algorithmic bytes / HBM peak, algorithmic flops / fp64 peak); the
            # larger of the two bounds is the roof it is measured against, the other one is reported beside it
            sec = kern["fused_chain_tsqr"]["avg_ms"] * 1e-3 * launches_per_step["fused_chain_tsqr"]
            gbs = bytes_per_sample * N / sec / 1e9
            tfs = flops_per_sample * N / sec / 1e12
            kept = np.array([meta["names_std"].index(p) for p in out["params_r"]])
            first = np.searchsorted(kept, 14 * np.arange(rows_per_sample))
            ex_flops = int(sum(2 * (n_kept + 1 - f) ** 2 for f in first))
            hbm_bound = gbs / HBM_PEAK_GBS >= tfs / FP64_PEAK_TFLOPS
            roof["fused_chain_tsqr"] = {
                "bound": "hbm" if hbm_bound else "fp64",
                "achieved": gbs if hbm_bound else tfs, "peak": HBM_PEAK_GBS if hbm_bound else FP64_PEAK_TFLOPS,
                "unit": "GB/s" if hbm_bound else "TFLOP/s", "traffic": None,
                "algorithmic_bytes_per_sample": bytes_per_sample, "algorithmic_flops_per_sample": flops_per_sample,
                "executed_flops_per_sample": ex_flops,
                "hbm": {"achieved_GBps": gbs, "frac": gbs / HBM_PEAK_GBS},
                "fp64": {"achieved_TFLOPs": tfs, "frac": tfs / FP64_PEAK_TFLOPS, "executed_TFLOPs": ex_flops * N / sec / 1e12,
                         "pipe": "fp64 VALU (v_fmac_f64 with a DPP row_newbcast operand; no MFMA instruction is issued -- "
                                 "v_mfma_f64_16x16x4 has the same 78.6 TFLOP/s peak and shares the FP64 datapath)"},
                "what": "regressor rows produced by two waves per CU into LDS tiles, streamed to W (every byte of the 6N x 84 "
                        "matrix written in every pass), each tile factored out of LDS by one of six consumer waves: W is not "
                        "read back"}
        if "tsqr" in kern:
            sec = kern["tsqr"]["avg_ms"] * 1e-3 * launches_per_step["tsqr"]
            roof["tsqr"] = {"bound": "fp64", "achieved": flops_per_sample * N / sec / 1e12, "peak": FP64_PEAK_TFLOPS,
                            "unit": "TFLOP/s", "traffic": None, "algorithmic_flops_per_sample": flops_per_sample}
            if n_kept + 1 <= 80:
                roof["tsqr"]["pipe"] = ("fp64 VALU (v_fmac_f64 with a DPP row_newbcast operand, no MFMA instruction is issued): "
                                        "v_mfma_f64_16x16x4 has the same 78.6 TFLOP/s peak and shares the FP64 datapath "
                                        "(tools/microbench/latency.hip), so that peak is the roof of this kernel")
                # the kernel skips the structurally zero leading columns of each joint's row block (structure hint): the
                # flops it executes are 2 (nc - first_j)^2 per row of block j, not the dense 2 nc^2
                kept = np.array([meta["names_std"].index(p) for p in out["params_r"]])
                first = np.searchsorted(kept, 14 * np.arange(rows_per_sample))
                roof["tsqr"]["executed_flops_per_sample"] = int(sum(2 * (n_kept + 1 - f) ** 2 for f in first))
            else:
                roof["tsqr"]["pipe"] = ("fp64 matrix pipe: 16-column panels on the VALU, compact-WY trailing updates as "
                                        "v_mfma_f64_16x16x4 (figh_tsqr_wide.hip); rows whose leading columns are zero start "
                                        "at their first non-zero column, so the executed flops are below the dense 2 m n^2")
                blocks = getattr(pipe, "_block_cache", None) if getattr(pipe, "_tree_blocks", False) else None
                if blocks is not None:
                    # joint-torque regressor of a tree: every row block is factored over the columns of its joint's subtree only
                    # (figh_tsqr_selected_blocks).  The reference's dense count 2 m n^2 is then 40 x the flops this path is
                    # asked to execute, so `achieved` / `frac` are restated on the EXECUTED flops (they would exceed the peak
                    # otherwise) and the dense-equivalent rate is kept beside them.
                    ex = int(sum(2 * (int(c) + 1) ** 2 for c in blocks[1]))
                    roof["tsqr"]["algorithmic_equivalent_TFLOPs"] = roof["tsqr"]["achieved"]
                    roof["tsqr"]["executed_flops_per_sample"] = ex
                    roof["tsqr"]["achieved"] = ex * N / sec / 1e12
                    roof["tsqr"]["launches_per_step"] = launches_per_step["tsqr"]
                    roof["tsqr"]["pipe"] += ("; per-row-block column lists: `achieved` counts the executed flops "
                                             "sum_j 2 (n_j + 1)^2 per sample, the launches are 24 small ones (7 .. 86 columns)")
                if getattr(pipe, "_wrench_split", False) and getattr(pipe, "_nf_expected", 0) > 0:
                    # external wrench on a free-flyer root: the three force row blocks are factored over the nf columns that
                    # can be non-zero there (figh_tsqr_selected_wrench) -- `achieved` above counts the reference's dense
                    # 2 m n^2, the flops this path is asked to execute are fewer
                    nf = pipe._nf_expected
                    roof["tsqr"]["executed_flops_per_sample"] = int(3 * 2 * (nf + 1) ** 2 + 3 * 2 * (n_kept + 1) ** 2)
                    roof["tsqr"]["executed_TFLOPs"] = roof["tsqr"]["executed_flops_per_sample"] * N / sec / 1e12
                    roof["tsqr"]["frac_executed"] = roof["tsqr"]["executed_TFLOPs"] / FP64_PEAK_TFLOPS
                    roof["tsqr"]["launches_per_step"] = launches_per_step["tsqr"]
                    # (the fraction of the roof is the one on the flops the kernels are asked to execute; the rate
                    # on the reference's dense 2 m n^2 is kept beside it and is not a fraction of anything)
                    roof["tsqr"]["dense_equivalent_TFLOPs"] = roof["tsqr"]["achieved"]
                    roof["tsqr"]["achieved"] = roof["tsqr"]["executed_TFLOPs"]
        # HBM bytes per launch: PMC counters cannot be read from inside the process -- the number below comes from the
        # committed rocprofv3 --pmc passes of this same command (FETCH_SIZE x2 as the gfx950 correction + WRITE_SIZE,
        # tools/pmc_summary.py), i.e. from the builder's run, not from this one
        try:
            pmc_file = next(n for n in ("r06_pmc_summary.json", "r05_pmc_summary.json", "r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json")
                            if os.path.exists(os.path.join(ROOT, "profiles", n)))
            with open(os.path.join(ROOT, "profiles", pmc_file)) as f:
                pmc = json.load(f)
            if args.config == "cfg2" and N == 1_000_000:
                for key, kname in (("regressor_chain", "regressor_chain_kernel<6, false, true>"),
                                   ("tsqr", "tsqr2_kernel<4, 4, true>"), ("fused_chain_tsqr", "fused_chain_tsqr_kernel<6>")):
                    if key in roof and kname in pmc and "hbm_bytes" in pmc[kname]:
                        roof[key]["traffic"] = pmc[kname]["hbm_bytes"]
                        roof[key]["traffic_source"] = ("profiles/%s: a committed rocprofv3 --pmc run of this command, NOT "
                                                       "measured in this run" % pmc_file)
            if args.config == "cfg4" and N == 4_000_000:
                pmc4 = next(n for n in ("r06_pmc_summary_cfg4.json", "r05_pmc_summary_cfg4.json", "r04_pmc_summary_cfg4.json", "r03_pmc_summary_cfg4.json", "r02_pmc_summary_cfg4.json")
                            if os.path.exists(os.path.join(ROOT, "profiles", n)))
                with open(os.path.join(ROOT, "profiles", pmc4)) as f:
                    pmc = json.load(f)
                src = "profiles/%s: a committed rocprofv3 --pmc run of this command, NOT measured in this run" % pmc4
                wy = next((n for n in ("tsqr_wy_kernel<4, 5, 4, 2, true, 0>", "tsqr_wy_kernel<4, 5, 4, 2, true>") if n in pmc), "")
                k1p = next((n for n in ("regressor_tape_kernel<16, true, true, true, true, true>",
                                        "regressor_tape_kernel<16, true, true, true, true>") if n in pmc), "")
                for key, kname in (("regressor_tree", k1p), ("tsqr", wy)):
                    if key in roof and kname in pmc and "hbm_bytes" in pmc[kname]:
                        roof[key]["traffic"] = pmc[kname]["hbm_bytes"]
                        roof[key]["traffic_source"] = src + (" (the torque-row launch of the two level-0 launches)" if key == "tsqr" else "")
                k = pmc.get(wy, {})
                if "tsqr" in roof and "SQ_INSTS_VALU_MFMA_MOPS_F64" in k:
                    # one MOPS unit = 512 flops (4 units per v_mfma_f64_16x16x4 = 2048 flops, checked against SQ_INSTS_MFMA)
                    roof["tsqr"]["executed_mfma_flops_per_launch"] = 512.0 * k["SQ_INSTS_VALU_MFMA_MOPS_F64"]
                    roof["tsqr"]["mfma_counters_source"] = src
        except Exception:
            pass
        for r in roof.values():
            r["frac"] = r["achieved"] / r["peak"]
        main_k = {k: v for k, v in kern.items() if "launches" in v}
        dominant = max(main_k, key=lambda k: main_k[k]["avg_ms"] * main_k[k]["launches"]) if main_k else None
        if rank == 0:
            line = {
                "metric": "samples/sec regressor build + TSQR solve, UR10 6-DoF" if args.config == "cfg2" else
                          "samples/sec regressor build + TSQR solve, %s" % model_name,
                "value": n_total * steps / dt,
                "unit": "samples/s",
                "n_gpus": world,
                "steps": steps,
                "warmup": warmup,
                "ms_per_step": 1e3 * dt / steps,
                "ms_per_step_median": 1e3 * float(np.median(step_times)),
                "ms_per_step_min": 1e3 * float(np.min(step_times)),
                "ms_first_pass": 1e3 * float(np.median(first_times)),
                "higher_is_better": True,
                "scaling": scaling,
                "vs_baseline": None,
                "dtype": "f64",
                "data": "synthetic",
                "config": {
                    "workload": {
                        "cfg2": "BASELINE configs[1]: UR10 6-DoF, %d synthetic (q,qd,qdd) samples per GPU, full inertial "
                                "regressor materialised (6N x 84) + elimination + Householder TSQR base params + LS" % N,
                        "cfg3": "BASELINE configs[2]: TIAGo, fv/fs + actuator inertia + offset columns, %d samples in total, "
                                "regressor (24N x 336, device-resident, link-padded) + elimination + blocked TSQR + LS%s" % (
                                    n_total, " + WLS solve (per-joint variances from the OLS residuals, weighted factorisation "
                                    "of the per-row-block triangles: %s)" % out.get("wls_source", "") if wls else
                                    " (WLS left out: --no-wls)"),
                        "cfg4": "BASELINE configs[3]: TALOS floating base, external-wrench regressor, %d samples in total "
                                "sharded over the GPUs, regressor (6N x 462, device-resident, link-padded) + blocked TSQR" % n_total,
                        "cfg5": "BASELINE configs[4]: human whole-body, %d samples in total sharded over the GPUs, %s" % (
                            n_total, ("streamed in chunks of %s samples (W never exists in full)" % chunk) if chunk else
                            "external-wrench regressor (6N x 560) device-resident in the link-compact layout (19 links with "
                            "mass x 16 columns) + force / torque split TSQR"),
                    }[args.config],
                    "samples_this_rank": N, "samples_total": n_total, "columns": ncols, "kept_columns": n_kept,
                    "base_parameters": len(out["idx_base"]), "collective": xinfo["collective"], "ranks": world,
                    "rank0_seconds": dt_rank, "max_rank_seconds": dt,
                    "device": _lib.device_info()["name"], "result_matches_reference": bool(ok),
                    "figh_env": "none set (checked)", "host_wait": host_wait,
                    "w_placement": pipe.placement_report or {"trials": 1},
                    "w_layout": ("block-compact: row block j = N x 16 |subtree_j| (%.1f GB instead of %.1f GB)"
                                 % (8e-9 * pipe.N * float(pipe._compact[1].sum()), 8e-9 * pipe.W.rows * pipe.W.ld))
                    if getattr(pipe, "_compact", None) is not None else (
                        ("force-compact: force rows %d columns (one line per four links) in front of the torque rows' %d%s; %.1f GB resident"
                         % (pipe._force_ld, pipe.W.ld, (", link-compact: %d of %d links have columns" % (
                             int((pipe._link_pos >= 0).sum()), len(pipe._link_pos))) if getattr(pipe, "_link_pos", None) is not None else "",
                            8e-9 * pipe.W.buf.size))
                        if getattr(pipe, "_force_ld", 0) else (
                            "link-compact: %d of %d links have columns (%.1f GB resident)" % (
                                int((pipe._link_pos >= 0).sum()), len(pipe._link_pos), 8e-9 * pipe.W.rows * pipe.W.ld)
                            if getattr(pipe, "_link_pos", None) is not None else "dense")),
                    "active_row_blocks": row_blocks,
                    "structural_zeros": args.structural_zeros + (" (in effect)" if getattr(pipe, "_zeros_once", False) else ""),
                    "null_pivots": ("on: columns null to tol_qr / 64 skip their column steps (figh_tsqr_null_pivot_tol); every pass "
                                    "certified against plain Householder afterwards (_host.null_rule_certified)"
                                    if pipe.null_pivots else (
                                        "off: a pass could not be certified (pivot close to tol_qr) and was repeated without the rule; "
                                        "the rule stays off (fallbacks: %d)" % pipe.null_rule_fallbacks
                                        if getattr(pipe, "null_rule_fallbacks", 0) else "off")),
                    "pivots": {"dependent_max": float(np.max(np.delete(out["absdiagR"], out["idx_base"]), initial=0.0)),
                               "base_min": float(np.min(np.asarray(out["absdiagR"])[out["idx_base"]])), "tol_qr": pipe.tol_qr},
                    "fused": ("K1 + level-0 TSQR in one launch (figh_regressor_tsqr_fused), %d of the %d timed and warm-up passes"
                              % (pipe.fused_passes, steps + warmup + 7) +
                              "; first passes (kept set from a 4096-sample prefix): %d of 5 fused" % first_fused) if pipe.fused_passes else
                             "no (two launches: W written by K1, read back by the TSQR)",
                },
                "roofline": dict(roof.get(dominant, {}), kernel=dominant) if dominant in roof else None,
                "kernels": {k: dict(kern[k], **roof.get(k, {})) for k in kern},
                "transfers": transfers,
            }
            if with_cpu and world == 1 and args.config in ("cfg2", "cfg3"):
                n_cpu = args.cpu_samples or (300000 if args.config == "cfg2" else 20000)
                line["cpu_baseline"] = cpu_baseline(robot, args.config, param, 7, n_cpu, n_config)
                line["cpu_baseline_fast"] = cpu_baseline_fast(robot, args.config, param, 7, n_cpu, n_config)
                # BASELINE.md holds no published number for this metric; the ratio asked for is the one to the CPU path of
                # the same pass measured in this run (fair-fast port; the faithful reference structure beside it)
                # (`vs_baseline` stays null: the contract reserves it for a published number)
                line["vs_cpu_baseline"] = {"fair_fast": line["value"] / line["cpu_baseline_fast"]["value"],
                                           "faithful_reference_structure": line["value"] / line["cpu_baseline"]["value"],
                                           "note": "ratios of `value` to the two CPU legs of THIS run; north_star's target is "
                                                   ">= 50x over the faithful one"}
        pipe = None  # (HBM back before the next config is set up)
        return (line if rank == 0 else None), ok

    line, ok = measure(args, args.steps, args.warmup, not args.no_cpu_baseline, dump_dir=args.dump_outputs)
    if args.strong_config and args.strong_config != args.config and ok:
        # north_star words its scaling target as STRONG scaling ("\u2265 6x at 8 GPUs"); the headline workload above is quoted
        # per GPU (weak).  So the same line carries a fixed-total-size measurement of a sharded BASELINE config (default
        # cfg4: TALOS, 4e6 samples in total, contiguous shards) at every N, N = 1 included: value(N) / value(1) of THIS
        # object is the strong-scaling curve
        import argparse as _ap
        sargs = _ap.Namespace(**dict(vars(args), config=args.strong_config, scaling="strong", samples=args.strong_samples,
                                     chunk_samples=None, active_joints=False))
        try:
            sline, sok = measure(sargs, args.strong_steps, 2, False)
            if rank == 0:
                line["strong_scaling"] = {k: sline[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step",
                                                                "ms_per_step_median", "scaling")}
                line["strong_scaling"]["config"] = {k: sline["config"][k] for k in (
                    "workload", "samples_this_rank", "samples_total", "collective", "ranks", "result_matches_reference",
                    "max_rank_seconds", "w_layout")}
                line["strong_scaling"]["kernels"] = {k: {kk: vv for kk, vv in v.items() if kk in ("launches", "launches_per_step", "avg_ms")}
                                                     for k, v in sline["kernels"].items()}
            ok = ok and sok
        except Exception as e:  # noqa: BLE001  (the headline measurement stands on its own)
            if world > 1:
                raise  # a rank that leaves a collective pass alone would leave its peers waiting
            line["strong_scaling"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    if rank == 0:
        print(json.dumps(line))
    if world > 1:
        barrier()
        if hasattr(exchange, "close"):
            exchange.close()
    if not ok:
        raise SystemExit("bench.py: the step did not reproduce the reference's structural result (idx_e / idx_base / "
                         "expressions) -- the line above is not a valid measurement")


def spawn_ranks(n):
    """``python bench.py --gpus N`` without a launcher (WORLD_SIZE unset): start N FRESH child processes of this script, one
    per rank, with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in their environment (what
    torch.distributed.run would set; the ranks meet over figaroh_plus_amd.dist.SocketGroup, so no PyTorch is involved), relay
    their output and return the worst exit code.  The parent never loads the library or touches the GPU: nothing that has
    initialised HIP is ever re-executed.  LOCAL_RANK modulo the device count picks the device; on a box with fewer GPUs
    than ranks the ranks share devices and the exchange negotiates itself down to the host-staged one
    (dist.exchange_from_env), which the line reports in config.collective."""
    import socket
    import subprocess

    port = None
    for _ in range(50):  # (MASTER_PORT and MASTER_PORT + 101, where the socket control plane listens, both free)
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            cand = s.getsockname()[1]
        try:
            with socket.socket() as s2:
                s2.bind(("127.0.0.1", cand + 101))
            port = cand
            break
        except (OSError, OverflowError):
            continue
    if port is None:
        raise SystemExit("bench.py: no free port pair for the rank processes")
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    worst = 0
    try:
        # (the children write to this process's stdout / stderr themselves: rank 0 prints the line)
        while any(p.poll() is None for p in procs):
            time.sleep(0.05)
            failed = [p.returncode for p in procs if p.poll() is not None and p.returncode != 0]
            if failed and not worst:
                worst = failed[0]
                time.sleep(2.0)  # peers that fail for the same reason get to say so themselves ...
                for other in procs:  # ... the rest would wait for the dead rank at the next exchange for ever
                    if other.poll() is None:
                        other.terminate()
        worst = worst or next((p.returncode for p in procs if p.returncode != 0), 0)
    except BaseException:
        for p in procs:
            if p.poll() is None:
                p.kill()
        raise
    return worst if worst >= 0 else 1


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out, path):
    """The numeric entries of one pass's result (IdentificationPipeline.run: index lists, regrouping coefficients, column
    norms, pivots, phi, ...) as path/<key>.npy in float64; the expression strings are left out.  Every entry is a few
    hundred numbers at most (they scale with the column count, not the samples), so nothing needs to be sampled.
    Two runs agree up to rounding, not bit for bit, in what comes from the triangle (absdiagR, phi_ls, residual_norm):
    which consumer wave factors which tile is decided at run time (the fused launch)."""
    arrays = {}
    for key, val in sorted(out.items()):
        if val is None or isinstance(val, str):
            continue
        arr = np.asarray(val)
        if arr.dtype.kind in "biuf":
            arrays[key] = np.array(arr, dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py --dump-outputs: %d bytes of outputs, more than the %d allowed" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for key, arr in arrays.items():
        np.save(os.path.join(path, key + ".npy"), arr)


def meta_idx(meta):
    names = meta["params_r"]
    base_first = [p.split(" ")[0] for p in meta["params_base"]]
    return [names.index(b) for b in base_first]


if __name__ == "__main__":
    main()
