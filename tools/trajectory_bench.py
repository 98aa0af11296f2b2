#!/usr/bin/env python3
"""Excitation loop with device-resident trajectories against the host-generated route.

    trajectory_bench.py [--pairs 3] [--out profiles/trajectory.json]

Per shape -- UR10 with B in {1, 8, 64, 256} trajectories of 1000 samples (5 waypoints), TIAGo's eight script joints with
B = 64 x 451 (10 waypoints) -- three alternating pairs in one process of
  (A) excitation.evaluate_waypoints_batch: waypoints up, figh_spline_sample, the batched objective and inverse dynamics on
      the resident samples, figh_excitation_constraints, (B, n_con) and B triangles down;
  (B) the route without resident trajectories: every trajectory from the vectorised NumPy mirror (CubicSpline.get_full_config;
      the reference's generator makes three ndcurves calls per sample and is not available here), objective_cond_batch and
      calc_torque_batch on the lists (concatenate + upload), tau down, constraint vectors sliced on the host.
Wall time per call (host clock around calls that end in a device-to-host copy; each measurement repeats the call until about
0.3 s have passed).  Separately, with the library's event pairs on: device time of figh_spline_sample (family "spline_sample":
the waypoint upload's tail, the coefficient launch and the sample launch), the 8 (nq + 2 nv) bytes per sample it has to write
and the fraction of the achievable HBM rate (6.3 TB/s) that makes.  (A) and (B) are also compared: constraint vectors bit for
bit, condition numbers to 1e-9."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from figaroh_plus_amd import _lib  # noqa: E402
from figaroh_plus_amd.tools import excitation as ex  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s
FREQ = 100
TIAGO_JOINTS = ["torso_lift_joint", "arm_1_joint", "arm_2_joint", "arm_3_joint", "arm_4_joint", "arm_5_joint", "arm_6_joint",
                "arm_7_joint"]


def golden(cfg):
    with open(os.path.join(ROOT, "tests", "golden", cfg + ".json")) as f:
        meta = json.load(f)
    return meta["param"], np.load(os.path.join(ROOT, "tests", "golden", cfg + ".npz"))


def indices_from_spline(robot, joints, param):
    """get_idx_b_cubic (examples/tiago/optimal_trajectory.py:72-94) at 10 waypoints: base columns of an active-joint spline."""
    from figaroh_plus_amd.tools.qrdecomposition import get_baseIndex
    from figaroh_plus_amd.tools.regressor import build_regressor_basic, build_regressor_reduced, get_index_eliminate
    cs = ex.CubicSpline(robot, 10, joints)
    rng = np.random.default_rng(40)
    wps, vel, acc = (s * rng.uniform(-1, 1, size=cs.dim_q) for s in (1.5, 2.0, 5.0))
    _, p, v, a = cs.get_full_config(FREQ, np.array([[0.5 * i] for i in range(10)]), wps, vel, acc)
    W = build_regressor_basic(robot, p, v, a, param)
    idx_e, par_r = get_index_eliminate(W, robot.get_standard_parameters(param), tol_e=0.001)
    return idx_e, get_baseIndex(build_regressor_reduced(W, idx_e), par_r)


def host_route(robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base):
    n_act, n_wps = cs.dim_q
    wps = ex.waypoints_from_search_variables(X, wp_init, n_wps, n_act)
    trajs, t = [], None
    for b in range(len(wps)):
        t, p, v, a = cs.get_full_config(FREQ, tps, wps[b], vel, acc)
        trajs.append((p, v, a))
    conds = ex.objective_cond_batch(robot, trajs, param, idx_e, idx_base)
    tau = ex.calc_torque_batch(robot, trajs, param)
    cons = np.array([ex.constraint_vector(cs, t, trajs[b][0], trajs[b][1], tau[b], tps) for b in range(len(wps))])
    return conds, cons


def timed(fn):
    """Seconds per call: one call to size the repeat count, then calls until about 0.3 s have passed."""
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    reps = max(1, min(50, int(0.3 / max(first, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps, reps


def measure(tag, robot, joints, tps, B, param, idx_e, idx_base, pairs):
    cs = ex.CubicSpline(robot, len(tps), joints)
    n_act, n_wps = cs.dim_q
    rng = np.random.default_rng(B)
    wp_init = rng.uniform(-0.5, 0.5, size=n_act)
    X = rng.uniform(-1.0, 1.0, size=(B, (n_wps - 1) * n_act))
    vel, acc = np.zeros((n_act, n_wps)), np.zeros((n_act, n_wps))  # gen_rand_wp's zero arrays, as the script runs
    tps = np.array(tps).reshape(-1, 1)

    def run_a():
        return ex.evaluate_waypoints_batch(robot, cs, FREQ, tps, X, vel, acc, wp_init, param, idx_e, idx_base)

    def run_b():
        return host_route(robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base)

    (ca, va), (cb, vb) = run_a(), run_b()  # warm-up of both, and the comparison
    same = bool(np.array_equal(va, vb))
    cond_rel = float(max(abs(x - y) / y for x, y in zip(ca, cb)))
    wall_a, wall_b, reps = [], [], []
    for _ in range(pairs):
        ta, ra = timed(run_a)
        tb, rb = timed(run_b)
        wall_a.append(1e3 * ta)
        wall_b.append(1e3 * tb)
        reps.append([ra, rb])
    m = robot.model
    wps = ex.waypoints_from_search_variables(X, wp_init, n_wps, n_act)
    _lib.profile_enable(True, 2)
    ms = []
    for k in range(6):
        _lib.profile_reset()
        batch = ex.spline_batch(cs, FREQ, tps, wps, vel, acc)
        _lib.synchronize()
        if k:
            ms.append(_lib.profile_get("spline_sample")[1])
    _lib.profile_enable(False)
    n_per = batch.n_per
    nbytes = 8 * (m.nq + 2 * m.nv) * B * n_per
    out = {"shape": tag, "B": B, "n_per": n_per, "n_wps": n_wps, "n_act": n_act, "nq": m.nq, "nv": m.nv, "base_columns": len(idx_base),
           "wall_ms_resident": wall_a, "wall_ms_host_route": wall_b, "calls_per_measurement": reps,
           "speedup_median": float(np.median(wall_b) / np.median(wall_a)),
           "constraints_bit_equal": same, "cond_max_rel_diff": cond_rel,
           "spline_sample": {"family": "spline_sample", "ms": ms, "bytes_written": nbytes,
                             "fraction_of_achievable_hbm": [nbytes / HBM_ACHIEVABLE / (t * 1e-3) for t in ms]},
           "bytes_over_the_bus_resident": 8 * (X.size + B * va.shape[1] + B * len(idx_base) ** 2),
           "bytes_over_the_bus_host_route": 8 * (B * n_per * (m.nq + 2 * m.nv) * 2 + B * n_per * m.nv + B * len(idx_base) ** 2)}
    print("%-12s B = %3d x %d: resident %s ms, host route %s ms, spline_sample %s ms (%.1f %% of 6.3 TB/s), same = %s, cond %.1e"
          % (tag, B, n_per, ["%.2f" % t for t in wall_a], ["%.2f" % t for t in wall_b], ["%.4f" % t for t in ms],
             100 * np.median(out["spline_sample"]["fraction_of_achievable_hbm"]), same, cond_rel), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trajectory.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("trajectory_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    shapes = []
    param, g = golden("cfg2_ur10")
    ur10 = Robot.from_flat("ur10")
    for B in (1, 8, 64, 256):
        shapes.append(measure("ur10", ur10, ur10.model.names[1:], [0.0, 2.5, 5.0, 7.5, 9.995], B, dict(param), g["idx_e"],
                              g["idx_base"], args.pairs))
    param, _ = golden("cfg3_tiago")
    tiago = Robot.from_flat("tiago")
    idx_e, idx_base = indices_from_spline(tiago, TIAGO_JOINTS, dict(param))
    shapes.append(measure("tiago_arm", tiago, TIAGO_JOINTS, [0.5 * i for i in range(10)], 64, dict(param), idx_e, idx_base,
                          args.pairs))
    report = {"tool": "tools/trajectory_bench.py --pairs %d" % args.pairs, "device": info["name"], "cu_count": info["cu_count"],
              "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
              "note": "wall_ms_*: host clock per call, (A) evaluate_waypoints_batch and (B) the host-generated route alternating; "
                      "spline_sample.ms: the library's event pair around the waypoint-table copy and both launches of "
                      "figh_spline_sample, one warm-up then five repeats; bytes_written: the q, v, a it has to store",
              "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
