#!/usr/bin/env python3
"""Self-collision distances of the excitation problem: figh_collision_distances against the NumPy mirror, and what the
collision rows add to one evaluate_waypoints_batch.

    collision_bench.py [--pairs P] [--batches 1,64,256] [--out profiles/collision.json]

TIAGo with the simplified collision model of tests/golden/tiago_simplified_collision.json (five objects, four pairs: box -
cylinder twice, cylinder - cylinder twice), the eight script joints, 10 waypoints half a second apart at 100 Hz: 451 samples
per trajectory, B trajectories from random waypoints inside the joint limits.
(a) the waypoint samples only, 9 B 4 queries, as the constraint vector asks for them; (b) every sample, 451 B 4 queries.
Per shape: device time of the entry by the library's own event pair (kernel family "collision_distances": the index upload
and the launch), queries per second, mean and maximum iteration count per pair and the statuses, and the wall time of
collision_distances_mirror on the same configurations (skipped above --mirror-max queries).
Then evaluate_waypoints_batch at the same B with collision=None and with the wrapper, wall time, alternating pairs in this
one process after a warm-up of each.  collision=None runs the statements the parent commit runs; the parent itself is not
built here.  The output carries the kernel's register / scratch / occupancy figures from the compiler's resource remarks."""
import argparse
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
from figaroh_plus_amd.tools import excitation as ex  # noqa: E402
from figaroh_plus_amd.tools import robotcollisions as rc  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

JOINTS = ["torso_lift_joint", "arm_1_joint", "arm_2_joint", "arm_3_joint", "arm_4_joint", "arm_5_joint", "arm_6_joint",
          "arm_7_joint"]
N_WPS, FREQ = 10, 100


def kernel_resources():
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_collision.hip"), "-o", os.devnull], capture_output=True, text=True)
    except OSError as e:
        return {"error": str(e)}
    out = {}
    for key, name in (("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("TotalSGPRs", "sgprs"), ("SGPRs Spill", "sgpr_spills"),
                      ("VGPRs Spill", "vgpr_spills"), ("ScratchSize \\[bytes/lane\\]", "scratch_bytes_per_lane"),
                      ("LDS Size \\[bytes/block\\]", "lds_bytes"), ("Occupancy \\[waves/SIMD\\]", "occupancy_waves_per_simd")):
        m = re.search(r"remark:\s+%s: (\d+)" % key, p.stderr)
        if m:
            out[name] = int(m.group(1))
    return out


def problem(B, seed=0):
    robot = Robot.from_flat("tiago")
    with open(os.path.join(ROOT, "tests", "golden", "tiago_simplified_collision.json")) as f:
        robot.geom_model = rc.GeometryModel.from_dict(json.load(f), robot.model)
    with open(os.path.join(ROOT, "tests", "golden", "cfg3_tiago.json")) as f:
        param = json.load(f)["param"]
    z = np.load(os.path.join(ROOT, "tests", "golden", "cfg3_tiago.npz"))
    cs = ex.CubicSpline(robot, N_WPS, JOINTS)
    rng = np.random.default_rng(seed)
    n_act = len(JOINTS)
    lo, up = np.maximum(cs.lower_q, -2.0), np.minimum(cs.upper_q, 2.0)
    wp_init = rng.uniform(lo, up)
    X = rng.uniform(np.tile(lo, N_WPS - 1), np.tile(up, N_WPS - 1), size=(B, (N_WPS - 1) * n_act))
    zeros = np.zeros((n_act, N_WPS))
    tps = [0.5 * i for i in range(N_WPS)]
    return robot, cs, param, z["idx_e"], z["idx_base"], tps, X, zeros, wp_init


def measure_entry(robot, batch, idx, pairs, mirror_max):
    gm = robot.geom_model
    P = len(gm.collisionPairs)
    n_eval = batch.n_per if idx is None else len(idx)
    nq = batch.B * n_eval * P
    out = _lib.DeviceArray((nq,), np.float64)
    st = _lib.DeviceArray((nq,), np.int32)

    def run():
        rc.collision_distances_device(robot, gm, batch.q.ptr, batch.q.ld, batch.B, batch.n_per, idx, out.ptr, n_eval * P,
                                      status_ptr=st.ptr)
    run()
    _lib.synchronize()
    times = []
    for _ in range(pairs):
        _lib.profile_reset()
        run()
        _lib.synchronize()
        times.append(_lib.profile_get("collision_distances")[1])
    s = st.to_host().reshape(-1, P)
    status, iters = s & 0xFFFF, s >> 16
    rec = {"B": batch.B, "samples_per_trajectory": n_eval, "queries": nq, "device_ms": times,
           "queries_per_s_best": nq / (min(times) * 1e-3),
           "iterations_mean_per_pair": iters.mean(axis=0).tolist(), "iterations_max_per_pair": iters.max(axis=0).tolist(),
           "status_counts_ok_intersect_cap": np.bincount(status.ravel(), minlength=3).tolist()}
    if nq <= mirror_max:
        q = batch.q.dense().buf.to_host().reshape(batch.B, batch.n_per, -1)
        q = q[:, idx if idx is not None else slice(None)].reshape(-1, q.shape[2])
        t0 = time.perf_counter()
        d = rc.collision_distances_mirror(robot.model, gm, q)[0]
        rec["mirror_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        rec["max_abs_diff_device_mirror"] = float(np.abs(d.reshape(-1) - out.to_host()).max())
    return rec


def measure_evaluate(problem_, pairs):
    robot, cs, param, idx_e, idx_base, tps, X, zeros, wp_init = problem_
    cw = rc.CollisionWrapper(robot)

    def run(collision):
        t0 = time.perf_counter()
        ex.evaluate_waypoints_batch(robot, cs, FREQ, tps, X, zeros, zeros, wp_init, param, idx_e, idx_base, collision=collision)
        return 1e3 * (time.perf_counter() - t0)
    run(None), run(cw)
    out = []
    for k in range(pairs):
        out.append({"pair": k + 1, "collision_none_wall_ms": run(None), "with_collision_wall_ms": run(cw)})
    none = [p["collision_none_wall_ms"] for p in out]
    return {"B": len(X), "pairs": out, "collision_none_spread_ms": max(none) - min(none),
            "added_by_collision_rows_ms_median": float(np.median([p["with_collision_wall_ms"] - p["collision_none_wall_ms"]
                                                                  for p in out]))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--mirror-max", type=int, default=120000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collision.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("collision_bench.py measures on a HIP device; none found")
    report = {"tool": "tools/collision_bench.py --pairs %d --batches %s" % (args.pairs, args.batches),
              "device": _lib.device_info()["name"],
              "note": "device_ms: the library's own event pair around the entry (index upload + launch); *_wall_ms: host wall "
                      "time; alternating pairs in one process after one warm-up of each route",
              "waypoint_samples": [], "every_sample": [], "evaluate_waypoints_batch": []}
    for B in (int(b) for b in args.batches.split(",")):
        pb = problem(B)
        robot, cs, _, _, _, tps, X, zeros, wp_init = pb
        wps = ex.waypoints_from_search_variables(X, wp_init, N_WPS, len(JOINTS))
        batch = ex.spline_batch(cs, FREQ, tps, wps, zeros, zeros)
        idx = ex.waypoint_sample_indices(batch.t, tps)
        assert batch.n_per == 451 and len(idx) == N_WPS - 1, (batch.n_per, idx)
        _lib.profile_enable(True, 2)
        report["waypoint_samples"].append(measure_entry(robot, batch, idx, args.pairs, args.mirror_max))
        report["every_sample"].append(measure_entry(robot, batch, None, args.pairs, args.mirror_max))
        _lib.profile_enable(False)
        report["evaluate_waypoints_batch"].append(measure_evaluate(pb, args.pairs))
        for key in ("waypoint_samples", "every_sample", "evaluate_waypoints_batch"):
            print(key, json.dumps(report[key][-1]), flush=True)
    report["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
