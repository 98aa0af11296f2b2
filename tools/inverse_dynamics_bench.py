#!/usr/bin/env python3
"""tau = W(q, v, a) . phi: the W-free entry against the route through a resident W, device time by HIP events.

    inverse_dynamics_bench.py [--samples N] [--pairs P] [--shapes ur10,tiago,talos] [--out profiles/inverse_dynamics.json]

(A) figh_regressor_apply (csrc/figh_dynamics.hip): one launch, kernel family "inverse_dynamics".
(B) the only route before ABI 108: the regressor into a resident W -- figh_regressor_build for the serial chain, the
    link-padded figh_regressor_build_padded for the trees -- then figh_matvec over all columns; kernel families
    "regressor_chain" / "regressor_tree" and "matvec".
Shapes: UR10 and TIAGo joint torques, TALOS external wrench, 1e6 samples each.  Per shape one warm-up of both paths, then P
alternating A / B pairs in this one process; the times are those of the library's own event pairs (figh_profile_enable(2)).
The output also carries the registers / scratch / occupancy of the two kernels from the compiler's resource remarks
(hipcc -Rpass-analysis=kernel-resource-usage on csrc/figh_dynamics.hip) and the largest difference between the two paths'
results over the largest |tau| of the row block."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from figaroh_plus_amd import _lib  # noqa: E402
from figaroh_plus_amd.device import GpuMatrix  # noqa: E402
from figaroh_plus_amd.tools.randomdata import sample_inputs  # noqa: E402
from figaroh_plus_amd.tools.regressor import regressor_flags  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

SHAPES = {"ur10": False, "tiago": False, "talos": True}  # model -> external wrench


def kernel_resources():
    """{kernel: {vgprs, agprs, sgprs, scratch_bytes_per_lane, lds_bytes, occupancy_waves_per_simd}} of figh_dynamics.hip."""
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_dynamics.hip"), "-o", os.devnull], capture_output=True, text=True)
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
            cur = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).replace("void ", "").replace("figh::", "")
            out[cur] = {}
        elif cur and ":" in t:
            k, val = t.rsplit(":", 1)
            if k.strip() in keys:
                out[cur][keys[k.strip()]] = int(val)
    return out


def family_ms(names):
    return sum(_lib.profile_get(n)[1] for n in names)


def measure(name, wrench, N, pairs):
    robot = Robot.from_flat(name)
    m = robot.model
    nl = m.njoints - 1
    param = dict(is_joint_torques=not wrench, is_external_wrench=wrench, has_friction=True, has_actuator_inertia=True,
                 has_joint_offset=True, force_torque=["All"] if wrench else None)
    mode, flags, ft = regressor_flags(param)
    handle = robot.device_model()
    rows, ncols = handle.shape(mode, flags)
    rng = np.random.default_rng(0)
    q, v, a = sample_inputs(m, N, rng, 1.5, 2, 5)
    dq, dv, da = (_lib.DeviceArray.from_host(x.reshape(-1)) for x in (q, v, a))
    phi = np.array(list(robot.get_standard_parameters(dict(param, Ia=[0.1] * nl, fv=[0.5] * nl, fs=[0.3] * nl, off=[0.05] * nl)
                                                      ).values()), dtype=np.float64)
    d_phi = _lib.DeviceArray.from_host(phi)
    d_tau_a = _lib.DeviceArray((rows * N,), np.float64)
    d_tau_b = _lib.DeviceArray((rows * N,), np.float64)
    chain = handle.is_chain() and not wrench
    ls = 14 if chain else 16
    ldw = ls * nl
    W = GpuMatrix.empty(rows * N, ldw)
    ref_cols = np.arange(ncols)
    d_idx = None if chain else _lib.DeviceArray.from_host((16 * (ref_cols // 14) + ref_cols % 14).astype(np.int32))
    build_family = "regressor_chain" if chain else "regressor_tree"

    def run_a():
        assert _lib.regressor_apply(handle, mode, flags, ft, N, dq, dv, da, d_phi, d_tau_a)

    def run_b():
        if chain:
            _lib.regressor_build(handle, mode, flags, ft, N, dq, dv, da, W.buf, ldw)
        else:
            _lib.regressor_build_padded(handle, mode, flags, ft, N, dq, dv, da, W.buf, ldw)
        _lib.matvec(W.buf, rows * N, ldw, d_idx, ncols, d_phi, d_tau_b)

    run_a()
    run_b()
    _lib.synchronize()
    ta, tb = d_tau_a.to_host().reshape(rows, N), d_tau_b.to_host().reshape(rows, N)
    diff = float((np.abs(ta - tb).max(axis=1) / np.abs(tb).max(axis=1)).max())
    out = []
    for k in range(pairs):
        _lib.profile_reset()
        run_a()
        _lib.synchronize()
        a_ms = family_ms(["inverse_dynamics"])
        _lib.profile_reset()
        run_b()
        _lib.synchronize()
        build_ms, mv_ms = family_ms([build_family]), family_ms(["matvec"])
        out.append({"pair": k + 1, "apply_ms": a_ms, "build_ms": build_ms, "matvec_ms": mv_ms, "build_matvec_ms": build_ms + mv_ms})
        print("%-6s pair %d: apply %.3f ms | build %.3f + matvec %.3f = %.3f ms" % (name, k + 1, a_ms, build_ms, mv_ms, build_ms + mv_ms),
              flush=True)
    a_all, b_all = [p["apply_ms"] for p in out], [p["build_matvec_ms"] for p in out]
    return {"model": name, "mode": "external_wrench" if wrench else "joint_torques", "samples": N, "rows_per_sample": rows,
            "ncols": ncols, "w_layout": "reference (14 columns per link)" if chain else "link-padded (16 columns per link)",
            "w_bytes": 8 * rows * N * ldw, "input_output_bytes_per_sample": 8 * (m.nq + 2 * m.nv + rows), "pairs": out,
            "apply_ms_min_max": [min(a_all), max(a_all)], "build_matvec_ms_min_max": [min(b_all), max(b_all)],
            "speedup_worst_pair": min(b_all) / max(a_all), "max_rel_diff_between_paths": diff}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--shapes", default="ur10,tiago,talos")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inverse_dynamics.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("inverse_dynamics_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    _lib.profile_enable(True, 2)
    report = {"tool": "tools/inverse_dynamics_bench.py --samples %d --pairs %d --shapes %s" % (args.samples, args.pairs, args.shapes),
              "device": info["name"], "cu_count": info["cu_count"],
              "note": "device time of the library's own event pairs; (A) figh_regressor_apply, (B) regressor into a resident W + "
                      "figh_matvec over all columns; alternating pairs in one process after one warm-up of each path",
              "shapes": [measure(name, SHAPES[name], args.samples, args.pairs) for name in args.shapes.split(",")]}
    _lib.profile_enable(False)
    report["kernel_resources"] = kernel_resources()
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
