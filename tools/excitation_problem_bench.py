#!/usr/bin/env python3
"""One Ipopt iteration's derivatives of the excitation problem: ExcitationProblem against what a caller had before it.

    excitation_problem_bench.py [--pairs P] [--out profiles/excitation_problem.json]

(A) one derivative pass of tools.excitation.ExcitationProblem -- objective, gradient, constraints and jacobian at one new
    X -- with singular_values="device" and with singular_values="host";
(B) the same four results as a caller of evaluate_waypoints_batch gets them: a host-made stencil, one
    evaluate_waypoints_batch (B r x r triangles and B n_con rows come down, LAPACK on the host), host quotients.
Shapes: UR10, 5 waypoints x 1000 samples (n_var 24), both schemes; TIAGo's eight script joints, 10 waypoints x 451 samples
(n_var 72, r = 98) with the simplified collision model, 2-point.  Wall time of the whole call, (A device), (A host) and (B)
in turn in one process after a warm-up of each, a new X for every call (nothing is served from a cache); then each route
alone, back to back ("blocks").  Beside it, from
separate calls: the device time of figh_singular_values_batch alone by the library's event pair, the host
singular_values_batch on the same triangles, and the sweeps per matrix."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from figaroh_plus_amd import _host, _lib  # noqa: E402
from figaroh_plus_amd.tools import excitation as ex  # noqa: E402
from figaroh_plus_amd.tools import robotcollisions as rc  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

FREQ = 100
UR10_JOINTS = ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint", "wrist_3_joint"]
TIAGO_JOINTS = ["torso_lift_joint", "arm_1_joint", "arm_2_joint", "arm_3_joint", "arm_4_joint", "arm_5_joint", "arm_6_joint",
                "arm_7_joint"]


def setup(name):
    """(robot, spline, tps, X, vel, acc, wp_init, param, idx_e, idx_base, collision)"""
    cfg, model, joints, n_wps = (("cfg2_ur10", "ur10", UR10_JOINTS, 5) if name == "ur10" else
                                 ("cfg3_tiago", "tiago", TIAGO_JOINTS, 10))
    robot = Robot.from_flat(model)
    with open(os.path.join(ROOT, "tests", "golden", cfg + ".json")) as f:
        param = json.load(f)["param"]
    z = np.load(os.path.join(ROOT, "tests", "golden", cfg + ".npz"))
    cw = None
    if name == "tiago":
        with open(os.path.join(ROOT, "tests", "golden", "tiago_simplified_collision.json")) as f:
            robot.geom_model = rc.GeometryModel.from_dict(json.load(f), robot.model)
        cw = rc.CollisionWrapper(robot)
    cs = ex.CubicSpline(robot, n_wps, joints)
    idx_e, idx_base = z["idx_e"], z["idx_base"]
    if name == "tiago":
        # get_idx_from_random (optimal_trajectory.py:72-94): the eliminated and the base columns of a random spline of the
        # ACTIVE joints; the golden's indices come from a motion of every joint and are singular on an arm-only trajectory
        from figaroh_plus_amd.tools.qrdecomposition import get_baseIndex
        from figaroh_plus_amd.tools.regressor import build_regressor_basic, build_regressor_reduced, get_index_eliminate
        rng = np.random.default_rng(40)
        shape = (len(joints), n_wps)
        _, p, v, a = cs.get_full_config(FREQ, np.array([[0.5 * i] for i in range(n_wps)]), rng.uniform(-1.5, 1.5, size=shape),
                                        rng.uniform(-2.0, 2.0, size=shape), rng.uniform(-5.0, 5.0, size=shape))
        W = build_regressor_basic(robot, p, v, a, param)
        idx_e, par_r = get_index_eliminate(W, robot.get_standard_parameters(param), tol_e=0.001)
        idx_base = get_baseIndex(build_regressor_reduced(W, idx_e), par_r)
    rng = np.random.default_rng(3)
    lo, up = np.maximum(cs.lower_q, -1.5), np.minimum(cs.upper_q, 1.5)
    wp_init = rng.uniform(lo, up)
    X = rng.uniform(np.tile(lo, n_wps - 1), np.tile(up, n_wps - 1))
    zeros = np.zeros(cs.dim_q)
    tps = [0.0, 2.5, 5.0, 7.5, 9.995] if name == "ur10" else [0.5 * i for i in range(n_wps)]
    return robot, cs, tps, X, zeros, zeros, wp_init, param, idx_e, idx_base, cw


def measure(name, scheme, pairs):
    robot, cs, tps, X, vel, acc, wp_init, param, idx_e, idx_base, cw = setup(name)
    probs = {route: ex.ExcitationProblem(robot, cs, FREQ, tps, vel, acc, wp_init, param, idx_e, idx_base, collision=cw,
                                         scheme=scheme, singular_values=route) for route in ("device", "host")}
    count = [0]

    def new_x():
        count[0] += 1
        return X + 1e-4 * count[0]

    def run_problem(route):
        p, x = probs[route], new_x()
        t0 = time.perf_counter()
        p.gradient(x), p.jacobian(x), p.objective(x), p.constraints(x)  # (derivatives first: one derivative pass)
        return 1e3 * (time.perf_counter() - t0)

    def run_caller():
        x = new_x()
        t0 = time.perf_counter()
        h, dx = ex.finite_difference_steps(x, scheme)
        conds, rows = ex.evaluate_waypoints_batch(robot, cs, FREQ, tps, ex.finite_difference_stencil(x, h, scheme), vel, acc,
                                                  wp_init, param, idx_e, idx_base, collision=cw)
        ex.difference_quotients(np.asarray(conds)[:, None], dx, scheme), ex.difference_quotients(rows, dx, scheme)
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(2):
        run_problem("device"), run_problem("host"), run_caller()
    rounds = [{"pair": k + 1, "problem_device_wall_ms": run_problem("device"), "problem_host_wall_ms": run_problem("host"),
               "caller_wall_ms": run_caller()} for k in range(pairs)]
    # each route alone, back to back: a stall that follows the host route's LAPACK thread pool into the NEXT call (seen in
    # the alternating rounds on hosts with a CPU quota, _host.single_threaded_blas) cannot land on another route here
    blocks = {key: [fn() for _ in range(pairs)] for key, fn in (("problem_device_wall_ms", lambda: run_problem("device")),
                                                                  ("problem_host_wall_ms", lambda: run_problem("host")),
                                                                  ("caller_wall_ms", run_caller))}
    p = probs["device"]
    B, r = p.last_pass.B, p.r
    d_R = p._pass_buffers(B)[3]
    # the singular values alone, on the triangles of the last pass
    _lib.profile_enable(True, 2)
    dev = []
    for _ in range(pairs):
        _lib.profile_reset()
        _host.singular_values_batch_device(d_R, B, r)
        _lib.synchronize()
        dev.append(_lib.profile_get("singular_values_batch")[1])
    _lib.profile_enable(False)
    tri = np.triu(d_R.to_host().reshape(B, r, r))
    host, dev_wall = [], []
    for _ in range(pairs):
        t0 = time.perf_counter()
        with _host.single_threaded_blas():
            s_host = _host.singular_values_batch(tri)
        host.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        s_dev, sweeps, fallbacks = _host.singular_values_batch_device(d_R, B, r, return_status=True)
        dev_wall.append(1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median([x[k] for x in rounds])) for k in blocks}
    return {"robot": name, "scheme": scheme, "B": B, "n_per": p.n_per, "n_var": p.n_var, "n_con": p.n_con, "r": r,
            "rounds": rounds, "median_wall_ms": med, "blocks": blocks,
            "median_wall_ms_blocks": {k: float(np.median(v)) for k, v in blocks.items()},
            "singular_values": {"device_kernel_ms": dev, "device_call_wall_ms": dev_wall, "host_lapack_wall_ms": host,
                                "host_workers": min(B, max(1, _host.cpu_budget() // 2), 8),
                                "sweeps_min_median_max": (None if sweeps is None else  # (None: above 128 columns, host route)
                                                          [int(sweeps.min()), float(np.median(sweeps)), int(sweeps.max())]),
                                "host_fallbacks": int(fallbacks),
                                "max_rel_diff_sigma_min": float(np.abs(s_dev[:, -1] - s_host[:, -1]).max() / s_host[:, -1].min()),
                                "cond_first": float(s_host[0, 0] / s_host[0, -1])}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "excitation_problem.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("excitation_problem_bench.py measures on a HIP device; none found")
    report = {"tool": "tools/excitation_problem_bench.py --pairs %d" % args.pairs, "device": _lib.device_info()["name"],
              "note": "*_wall_ms: host wall time of the whole call (objective, gradient, constraints, jacobian at a new X), the "
                      "three routes in turn in one process after two warm-ups of each; device_kernel_ms: the library's event "
                      "pair around figh_singular_values_batch; host_lapack_wall_ms: _host.singular_values_batch on the same "
                      "downloaded triangles",
              "shapes": []}
    for name, scheme in (("ur10", "2-point"), ("ur10", "3-point"), ("tiago", "2-point")):
        report["shapes"].append(measure(name, scheme, args.pairs))
        print(json.dumps(report["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
