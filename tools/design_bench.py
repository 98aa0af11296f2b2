#!/usr/bin/env python3
"""D-optimal posture selection: the two device passes against the package's vectorised NumPy mirrors.

    design_bench.py [--pairs P] [--sizes 500,10000,1000000] [--out profiles/optimal_design.json]

TIAGo, head_2_joint -> a tool frame on arm_7_joint, full_params, all six components (c = 6).  The 34 base columns are chosen
on the 500 postures of tests/golden/tiago_calibration_pool_500.json (squared column norm >= 1e-6, then the columns whose
diagonal entry in np.linalg.qr exceeds 1e-8); N = 500 is that pool, larger pools are random_configurations.  The regressor
is built and restricted to the base columns on the device and stays there.

Per pass: device time of figh_design_gram (kernel family "design_gram": the tile launch and the reduction of the
partials) and of figh_design_scores ("design_scores": the upload of the factor and the launch, all three outputs) by the
library's own event pairs, each also as a fraction of 6.3 TB/s on the 8 c N n bytes of R read once.
(A) one multiplicative iteration on the device as SOCP.solve runs it (upload of w, Gram pass, host Cholesky, scores pass for
    the trace alone, download of the N traces), wall time;
(B) the same iteration on the NumPy mirrors (gram_mirror + scores_mirror), wall time.
One warm-up of each route, then P alternating pairs in this one process; one pair where (B) takes more than two seconds.
Whole solve: wall time of SOCP.solve(tol=1e-3) on the device at the largest size, its iteration count and the size of the
support (weights above 1e-5).  The output carries the kernels' register / scratch / LDS / occupancy figures from the
compiler's resource remarks."""
import argparse
import contextlib
import io
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from figaroh_plus_amd import _lib  # noqa: E402
from figaroh_plus_amd.calibration import calibration_tools as ct  # noqa: E402
from figaroh_plus_amd.calibration import optimal_design as od  # noqa: E402
from figaroh_plus_amd.device import GpuMatrix  # noqa: E402
from figaroh_plus_amd.model import SE3, rpy_to_matrix  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
C = 6


def kernel_resources():
    """{kernel: {vgprs, agprs, sgprs, scratch_bytes_per_lane, lds_bytes, occupancy_waves_per_simd}} of figh_design.hip (the
    scores kernels take their LDS at launch: 8 (NP (NP + 1) / 2 + 3072) bytes, plus 8 x 3456 of staging tiles up to NP = 80)."""
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_design.hip"), "-o", os.devnull], capture_output=True, text=True)
    except OSError as e:
        return {"error": str(e)}
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "lds_bytes", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(?:.*?:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = subprocess.run(["c++filt", t.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
            out[cur] = {}
        elif cur and ":" in t:
            k, val = t.rsplit(":", 1)
            if k.strip() in keys:
                out[cur][keys[k.strip()]] = int(val)
    return out


def make_case():
    m = Robot.from_flat("tiago").model
    m.addFrame("tool", m.getJointId("arm_7_joint"), SE3(rpy_to_matrix(0.3, -0.2, 0.5), [0.05, -0.02, 0.1]))
    sj, sp = ct._named_frame(m, "head_2_joint")
    ej, ep = ct._named_frame(m, "tool")
    return m, (ej, ep, sj, sp, ct.get_sup_joints(m, "head_2_joint", "tool"))


def fixture_configurations(m):
    with open(os.path.join(ROOT, "tests", "golden", "tiago_calibration_pool_500.json")) as f:
        d = json.load(f)
    cfg = np.array(d["calibration_joint_configurations"], dtype=np.float64)
    q = np.zeros((cfg.shape[0], m.nq))
    for j, name in enumerate(d["calibration_joint_names"]):
        q[:, m.joints[m.getJointId(name)].idx_q] = cfg[:, j]
    return q


def base_columns(m, frames, q):
    ej, ep, sj, sp, support = frames
    R, _ = ct.kinematic_regressor_batch(m, q, ej, ep, sj, sp, support, want_R=True, want_J=False)
    W = np.concatenate([R[:, k, :] for k in range(C)], axis=0)
    keep = [j for j in range(W.shape[1]) if np.sum(W[:, j] ** 2) >= 1e-6]
    Rq = np.linalg.qr(W[:, keep], mode="r")
    return [keep[k] for k in range(len(keep)) if abs(Rq[k, k]) > 1e-8]


def resident_pool(m, frames, q, cols):
    """The base regressor of the postures q, component-major, built and restricted to `cols` on the device."""
    ej, ep, sj, sp, support = frames
    N, width = len(q), 6 * (m.njoints - 1)
    d_q = GpuMatrix.from_host(q)
    full = GpuMatrix.empty(C * N, width)
    _lib.kinematic_regressor(_lib.ModelHandle(m.to_flat()), N, d_q.ptr, d_q.ld, ej, ct._placement12(ep), sj,
                             ct._placement12(sp), support, 63, full.ptr, full.ld, None, 0, None, None)
    Rb = GpuMatrix.empty(C * N, len(cols))
    _lib.gather_cols(full, C * N, full.ld, _lib.DeviceArray.from_host(np.asarray(cols, dtype=np.int32)), len(cols), Rb, Rb.ld)
    _lib.synchronize()
    return Rb


def measure(m, frames, q, cols, pairs):
    N, n = len(q), len(cols)
    Rb = resident_pool(m, frames, q, cols)
    pool = od.CandidatePool(Rb, N, C)
    host = Rb.numpy()
    w = np.full(N, 1.0 / N)

    only_d = (True, False, False)

    def run_a():
        return pool.scores(pool.information_matrix(w), want=only_d)[0]

    def run_b():
        M = od.gram_mirror(host, N, C, w)
        return od.scores_mirror(host, N, C, np.linalg.cholesky(M), want=only_d)[0]

    a = run_a()
    t0 = time.perf_counter()
    b = run_b()
    if time.perf_counter() - t0 > 2.0:
        pairs = 1
    diff = float(np.max(np.abs(a - b) / np.abs(b)))
    pool.scores(pool.information_matrix(w))  # (warm-up of the launch with all three outputs, which is what is timed below)
    out = []
    for k in range(pairs):
        _lib.profile_reset()
        pool.scores(pool.information_matrix(w))
        _lib.synchronize()
        gram_ms, scores_ms = _lib.profile_get("design_gram")[1], _lib.profile_get("design_scores")[1]
        t0 = time.perf_counter()
        run_a()
        a_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        run_b()
        b_ms = 1e3 * (time.perf_counter() - t0)
        out.append({"pair": k + 1, "gram_device_ms": gram_ms, "scores_device_ms": scores_ms, "iteration_device_route_wall_ms": a_ms,
                    "iteration_mirror_wall_ms": b_ms})
        print("N=%-8d pair %d: gram %.3f ms, scores %.3f ms | iteration: device route %.2f ms, mirror %.1f ms"
              % (N, k + 1, gram_ms, scores_ms, a_ms, b_ms), flush=True)
    nbytes = 8 * C * N * n
    g, s = [p["gram_device_ms"] for p in out], [p["scores_device_ms"] for p in out]
    return pool, {"candidates": N, "components": C, "columns": n, "bytes_of_R": nbytes, "pairs": out,
                  "gram_device_ms_min_max": [min(g), max(g)], "scores_device_ms_min_max": [min(s), max(s)],
                  "gram_fraction_of_6.3_TBps_best_pair": nbytes / (min(g) * 1e-3) / HBM_BYTES_PER_S,
                  "scores_fraction_of_6.3_TBps_best_pair": nbytes / (min(s) * 1e-3) / HBM_BYTES_PER_S,
                  "mirror_over_device_route_worst_pair":
                      min(p["iteration_mirror_wall_ms"] for p in out) / max(p["iteration_device_route_wall_ms"] for p in out),
                  "max_rel_diff_device_mirror_trace": diff}


def whole_solve(pool, max_iter):
    solver = od.SOCP(pool, {"NbSample": pool.N})
    t0 = time.perf_counter()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            w_list, _ = solver.solve(tol=1e-3, max_iter=max_iter)
        converged, support = True, int(np.sum(np.array(w_list) > 1e-5))
    except RuntimeError:
        converged, support = False, None
    return {"candidates": pool.N, "tol": 1e-3, "max_iter": max_iter, "converged": converged, "wall_s": time.perf_counter() - t0,
            "iterations": solver.iterations, "max_variance_over_n": solver.max_variance / pool.n,
            "efficiency_bound": solver.efficiency_bound, "weights_above_1e-5": support}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--sizes", default="500,10000,1000000")
    ap.add_argument("--max-iter", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimal_design.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("design_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    rng = np.random.default_rng(0)
    m, frames = make_case()
    q500 = fixture_configurations(m)
    cols = base_columns(m, frames, q500)
    _lib.profile_enable(True, 2)
    passes, solves = [], []
    sizes = [int(s) for s in args.sizes.split(",")]
    for N in sizes:
        q = q500 if N == len(q500) else ct.random_configurations(m, rng, N)
        pool, rec = measure(m, frames, q, cols, args.pairs)
        passes.append(rec)
        if N == len(q500) or N == max(sizes):
            _lib.profile_enable(False)
            solves.append(whole_solve(pool, args.max_iter))
            _lib.profile_enable(True, 2)
            print("solve N=%d: %s" % (N, solves[-1]), flush=True)
        del pool
    _lib.profile_enable(False)
    report = {"tool": "tools/design_bench.py --pairs %d --sizes %s --max-iter %d" % (args.pairs, args.sizes, args.max_iter),
              "device": info["name"], "base_columns": len(cols),
              "note": "*_device_ms: the library's own event pair around the entry's launches; *_wall_ms: host wall time; "
                      "alternating pairs in one process after one warm-up of each route (one pair where the mirror takes more "
                      "than two seconds)",
              "passes": passes, "whole_solve": solves, "kernel_resources": kernel_resources()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
