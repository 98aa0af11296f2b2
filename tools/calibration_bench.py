#!/usr/bin/env python3
"""Geometric calibration: the device entries against the package's own vectorised NumPy mirrors.

    calibration_bench.py [--pairs P] [--shapes ur10,tiago] [--sizes 1000,100000,1000000] [--out profiles/calibration.json]

Regressor, UR10 (universe -> tool on wrist_3) and TIAGo (torso_lift -> tool on arm_7), full_params, all six components:
(A) figh_kinematic_regressor into a resident R with the row sums of squares, device time of the library's own event pair
    (kernel family "kinematic_regressor": the memset of R and the launch);
(B) calibration_tools.kinematic_regressor_batch + the row stacking, wall time on the host;
and the public calculate_identifiable_kinematics_model with host arrays in and out on both routes, wall time (upload of q,
download of R and the host-side stacking included) -- the figure a crossover for host-array calls would have to come from.
FK batch, TIAGo, B x N = 64 x 500 and 64 x 1e5: (A) figh_calib_fkm_batch, device time; (B) fkm_pose_batch, wall time.
One warm-up of both routes per shape, then P alternating A / B pairs in this one process (one pair where the mirror's result
alone exceeds 1 GB).  The per-sample Python loop of the reference's structure (calculate_kinematics_model /
get_rel_kinreg per configuration) is timed once at 1e4 samples.  Bytes are inputs read once plus outputs written once, as
a fraction of 6.3 TB/s.  The output carries the kernels' register / scratch / LDS / occupancy figures from the compiler's
resource remarks."""
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
from figaroh_plus_amd.calibration import calibration_tools as ct  # noqa: E402
from figaroh_plus_amd.device import GpuMatrix  # noqa: E402
from figaroh_plus_amd.model import SE3, rpy_to_matrix  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPES = {"ur10": ("universe", "wrist_3_joint"), "tiago": ("torso_lift_joint", "arm_7_joint")}


def kernel_resources():
    """{kernel: {vgprs, sgprs, scratch_bytes_per_lane, lds_bytes, occupancy_waves_per_simd}} of figh_kinematics.hip."""
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_kinematics.hip"), "-o", os.devnull], capture_output=True, text=True)
    except OSError as e:
        return {"error": str(e)}
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
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


def make_case(name):
    start, end_joint = SHAPES[name]
    m = Robot.from_flat(name).model
    m.addFrame("tool", m.getJointId(end_joint), SE3(rpy_to_matrix(0.3, -0.2, 0.5), [0.05, -0.02, 0.1]))
    n = 1
    param = {"NbSample": n, "calibration_index": 6, "start_frame": start, "end_frame": "tool", "IDX_TOOL": m.getFrameId("tool"),
             "measurability": [True] * 6, "calib_model": "full_params", "q0": np.zeros(m.nq), "free_flyer": False,
             "config_idx": list(range(m.nq)), "param_name": [], "NbMarkers": 1}
    return m, param


def configurations(m, n, rng):
    q = rng.uniform(-1.5, 1.5, (n, m.nq))
    for jm in m.joints[1:]:
        if jm.jtype == 2:
            ang = rng.uniform(-np.pi, np.pi, n)
            q[:, jm.idx_q], q[:, jm.idx_q + 1] = np.cos(ang), np.sin(ang)
        elif jm.jtype == 1:
            q[:, jm.idx_q] = rng.uniform(0.0, 0.35, n)
    return q


def frames(m, param):
    if param["start_frame"] == "universe":
        ej, ep = ct._frame(m, param["IDX_TOOL"])
        return ej, ep, -1, None, ct._branch(m, ej)
    sj, sp = ct._named_frame(m, param["start_frame"])
    ej, ep = ct._named_frame(m, param["end_frame"])
    return ej, ep, sj, sp, ct.get_sup_joints(m, param["start_frame"], param["end_frame"])


def measure_regressor(name, N, pairs, rng):
    m, param = make_case(name)
    param["NbSample"] = N
    ej, ep, sj, sp, support = frames(m, param)
    q = configurations(m, N, rng)
    ncols = 6 * (m.njoints - 1)
    d_q = GpuMatrix.from_host(q)
    handle = _lib.ModelHandle(m.to_flat())
    R = GpuMatrix.empty(6 * N, ncols)
    sq = _lib.DeviceArray((6 * N,))

    def run_a():
        _lib.kinematic_regressor(handle, N, d_q.ptr, d_q.ld, ej, ct._placement12(ep), sj, ct._placement12(sp), support, 63,
                                 R.ptr, R.ld, None, 0, sq.ptr, None)

    def run_b():
        Rm, _ = ct.kinematic_regressor_batch(m, q, ej, ep, sj, sp, support, want_J=False)
        return np.ascontiguousarray(Rm.transpose(1, 0, 2)).reshape(6 * N, ncols)

    mirror_bytes = 8 * 6 * N * ncols
    if mirror_bytes > (1 << 30):
        pairs = 1
    run_a()
    _lib.synchronize()
    ref = run_b()
    got = R.numpy()
    diff = float(np.abs(got - ref).max())
    del got, ref
    out = []
    for k in range(pairs):
        _lib.profile_reset()
        run_a()
        _lib.synchronize()
        a_ms = _lib.profile_get("kinematic_regressor")[1]
        t0 = time.perf_counter()
        run_b()
        b_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        dev = ct.calculate_identifiable_kinematics_model(q, m, None, param)
        pub_dev_ms = 1e3 * (time.perf_counter() - t0)
        del dev
        out.append({"pair": k + 1, "device_ms": a_ms, "mirror_wall_ms": b_ms, "public_device_route_wall_ms": pub_dev_ms})
        print("%-6s N=%-8d pair %d: device %.3f ms | mirror %.1f ms | public call, device route, host in / out %.1f ms"
              % (name, N, k + 1, a_ms, b_ms, pub_dev_ms), flush=True)
    nbytes = 8 * (N * m.nq + 6 * N * ncols + 6 * N)
    a_all = [p["device_ms"] for p in out]
    return {"model": name, "start_frame": param["start_frame"], "samples": N, "ncols": ncols, "support_joints": len(support),
            "bytes_in_plus_out": nbytes, "pairs": out, "device_ms_min_max": [min(a_all), max(a_all)],
            "fraction_of_6.3_TBps_best_pair": nbytes / (min(a_all) * 1e-3) / HBM_BYTES_PER_S,
            "mirror_over_device_worst_pair": min(p["mirror_wall_ms"] for p in out) / max(a_all),
            "mirror_over_public_device_route_worst_pair":
                min(p["mirror_wall_ms"] for p in out) / max(p["public_device_route_wall_ms"] for p in out),
            "max_abs_diff_device_mirror": diff}


def measure_loop(name, N, rng):
    """The reference's structure: one Python call per configuration."""
    m, param = make_case(name)
    q = configurations(m, N, rng)
    t0 = time.perf_counter()
    for i in range(N):
        if param["start_frame"] == "universe":
            ct.calculate_kinematics_model(q[i], m, None, param)
        else:
            ct.get_rel_kinreg(m, None, param["start_frame"], param["end_frame"], q[i])
    return {"model": name, "samples": N, "per_sample_loop_wall_ms": 1e3 * (time.perf_counter() - t0)}


def measure_fkm(B, N, pairs, rng):
    m, param = make_case("tiago")
    param["NbSample"] = N
    support = ct.get_sup_joints(m, param["start_frame"], param["end_frame"])
    # arm_4 / arm_5 / arm_6 placements sit at gimbal lock (pitch -pi/2): not updated, as in a calibration of this arm
    act = [j for j in support if abs(ct.matrix_to_rpy(m.jointPlacements[j].rotation)[1]) < 1.5]
    param["actJoint_idx"] = act
    param["param_name"] = ["%s_%s" % (t, m.names[j]) for j in act for t in ct.FULL_PARAMTPL] + \
                          ["%s_1" % t for t in ct.EE_TPL]
    var = rng.uniform(-0.02, 0.02, (B, len(param["param_name"])))
    q = configurations(m, N, rng)
    chain, placements, wMo, eeMf = ct._fkm_tables(m, var, param)
    start, end = ct._named_frame(m, param["start_frame"]), ct._named_frame(m, param["end_frame"])
    d_q = GpuMatrix.from_host(q)
    d_t = [_lib.DeviceArray.from_host(t.reshape(-1)) for t in (placements, wMo, eeMf)]
    out_dev = GpuMatrix.empty(B, 6 * N)
    handle = _lib.ModelHandle(m.to_flat())

    def run_a():
        _lib.calib_fkm_batch(handle, B, N, d_q.ptr, d_q.ld, chain, d_t[0], d_t[1], d_t[2], end[0], ct._placement12(end[1]),
                             start[0], ct._placement12(start[1]), 63, out_dev.ptr, out_dev.ld)

    def run_b():
        return ct.fkm_pose_batch(m, q, chain, placements, wMo, eeMf, start, end, [True] * 6)

    run_a()
    _lib.synchronize()
    diff = float(np.abs(out_dev.numpy() - run_b()).max())
    out = []
    for k in range(pairs):
        _lib.profile_reset()
        run_a()
        _lib.synchronize()
        a_ms = _lib.profile_get("calib_fkm_batch")[1]
        t0 = time.perf_counter()
        run_b()
        b_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        ct.calc_updated_fkm_batch(m, None, var, q, param)
        pub_ms = 1e3 * (time.perf_counter() - t0)
        out.append({"pair": k + 1, "device_ms": a_ms, "mirror_wall_ms": b_ms, "public_device_route_wall_ms": pub_ms})
        print("fkm B=%d N=%-7d pair %d: device %.3f ms | mirror %.1f ms | public call, device route %.1f ms"
              % (B, N, k + 1, a_ms, b_ms, pub_ms), flush=True)
    nbytes = 8 * (N * m.nq + B * (len(chain) + 2) * 12 + B * 6 * N)
    a_all = [p["device_ms"] for p in out]
    return {"model": "tiago", "B": B, "N": N, "chain_joints": len(chain), "bytes_in_plus_out": nbytes, "pairs": out,
            "device_ms_min_max": [min(a_all), max(a_all)],
            "fraction_of_6.3_TBps_best_pair": nbytes / (min(a_all) * 1e-3) / HBM_BYTES_PER_S,
            "mirror_over_device_worst_pair": min(p["mirror_wall_ms"] for p in out) / max(a_all),
            "mirror_over_public_device_route_worst_pair":
                min(p["mirror_wall_ms"] for p in out) / max(p["public_device_route_wall_ms"] for p in out),
            "max_abs_diff_device_mirror": diff}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--shapes", default="ur10,tiago")
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("calibration_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    rng = np.random.default_rng(0)
    _lib.profile_enable(True, 2)
    sizes = [int(s) for s in args.sizes.split(",")]
    report = {"tool": "tools/calibration_bench.py --pairs %d --shapes %s --sizes %s" % (args.pairs, args.shapes, args.sizes), "device": info["name"],
              "note": "device_ms: the library's own event pair around the entry's launches; *_wall_ms: host wall time; "
                      "alternating pairs in one process after one warm-up of each route (one pair where the mirror's result "
                      "exceeds 1 GB)",
              "regressor": [measure_regressor(name, N, args.pairs, rng) for name in args.shapes.split(",") for N in sizes],
              "per_sample_loop": [measure_loop(name, 10000, rng) for name in args.shapes.split(",")],
              "fkm_batch": [measure_fkm(64, N, args.pairs, rng) for N in (500, 100000)]}
    _lib.profile_enable(False)
    report["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
