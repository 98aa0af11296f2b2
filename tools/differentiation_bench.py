#!/usr/bin/env python3
"""The device front end of the real-data chain -- finite differences and median filter -- device time by HIP events.

    differentiation_bench.py [--repeats R] [--baseline-samples B] [--out profiles/differentiation.json]

(1) figh_joint_difference + figh_gradient_cols (csrc/figh_differentiate.hip; kernel families "joint_difference",
    "gradient_cols"): the human model at 1e6 and 1e7 samples, UR10 at 1e6.
(2) figh_medfilt_cols (family "medfilt_cols"), kernel size 5, on 1e6 x 46.
(3) The baseline: the host path of calculate_first_second_order_differentiation (unchanged NumPy code) on the human model at
    B samples (default 1e4), wall clock on this machine's CPU; its per-sample cost and the LINEAR EXTRAPOLATION to the sizes of
    (1), stated as such.
Per launch the report carries the bytes it has to move -- 8 (nq + nv) per sample for the difference, 16 nv for the gradient,
16 per element for the median -- and the fraction of the achievable HBM rate (6.3 TB/s on the MI355X) that makes of the
measured time.  One warm-up, then R repeats; the times are those of the library's own event pairs (figh_profile_enable(2)).
The compiler's resource remarks of the translation unit are attached."""
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
from figaroh_plus_amd.identification.identification_tools import calculate_first_second_order_differentiation  # noqa: E402
from figaroh_plus_amd.tools.randomdata import sample_inputs  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s
TS = 0.01
BLOCK = 10 ** 6  # samples generated on the host; larger sets repeat this block on the device


def kernel_resources():
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_differentiate.hip"), "-o", os.devnull], capture_output=True, text=True)
    except OSError as e:
        return {"error": str(e)}
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "LDS Size [bytes/block]": "static_lds_bytes", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
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


def resident_positions(model, N):
    """N x nq device array: one host block of valid configurations, repeated on the device."""
    rng = np.random.default_rng(0)
    q, _, _ = sample_inputs(model, min(N, BLOCK), rng, 1.5, 2, 5)
    block = _lib.DeviceArray.from_host(np.ascontiguousarray(q).reshape(-1))
    if N <= BLOCK:
        return block
    d_q = _lib.DeviceArray((N * model.nq,), np.float64)
    lib = _lib.load()
    for lo in range(0, N, BLOCK):
        n = min(BLOCK, N - lo)
        _lib.check(lib.figh_memcpy_d2d(d_q.ptr + 8 * lo * model.nq, block.ptr, 8 * n * model.nq))
    return d_q


def entry(family, ms, nbytes):
    return {"family": family, "ms": ms, "bytes": nbytes,
            "fraction_of_achievable_hbm": [nbytes / HBM_ACHIEVABLE / (t * 1e-3) for t in ms]}


def measure_difference(name, N, repeats):
    model = Robot.from_flat(name).model
    handle = _lib.ModelHandle(model.to_flat())
    d_q = resident_positions(model, N)
    d_dq = _lib.DeviceArray(((N - 1) * model.nv,), np.float64)
    d_ddq = _lib.DeviceArray(((N - 1) * model.nv,), np.float64)
    diff_ms, grad_ms = [], []
    for k in range(repeats + 1):
        _lib.profile_reset()
        _lib.joint_difference(handle, N, d_q.ptr, TS, None, d_dq.ptr)
        _lib.gradient_cols(d_dq.ptr, N - 1, model.nv, model.nv, min(model.nq - 1, model.nv), TS, None, d_ddq.ptr, model.nv)
        _lib.synchronize()
        if k:  # (k == 0: warm-up)
            diff_ms.append(_lib.profile_get("joint_difference")[1])
            grad_ms.append(_lib.profile_get("gradient_cols")[1])
    print("%-6s N = %.0e: difference %s ms, gradient %s ms" % (name, N, ["%.3f" % t for t in diff_ms],
                                                                ["%.3f" % t for t in grad_ms]), flush=True)
    return {"model": name, "samples": N, "nq": model.nq, "nv": model.nv,
            "tile_pairs": _lib.joint_difference_tile(model.nq, model.nv),
            "joint_difference": entry("joint_difference", diff_ms, 8 * (model.nq + model.nv) * N),
            "gradient_cols": entry("gradient_cols", grad_ms, 16 * model.nv * (N - 1))}


def measure_medfilt(rows, cols, k, repeats):
    x = np.random.default_rng(1).normal(size=(rows, cols))
    d_x = _lib.DeviceArray.from_host(x.reshape(-1))
    d_y = _lib.DeviceArray((rows * cols,), np.float64)
    ms = []
    for i in range(repeats + 1):
        _lib.profile_reset()
        _lib.medfilt_cols(d_x.ptr, rows, cols, cols, 1, k, d_y.ptr, cols)
        _lib.synchronize()
        if i:
            ms.append(_lib.profile_get("medfilt_cols")[1])
    print("medfilt %d x %d, size %d: %s ms" % (rows, cols, k, ["%.3f" % t for t in ms]), flush=True)
    return dict(entry("medfilt_cols", ms, 16 * rows * cols), rows=rows, cols=cols, kernel_size=k)


def host_baseline(samples):
    model = Robot.from_flat("human").model
    q, _, _ = sample_inputs(model, samples, np.random.default_rng(2), 1.5, 2, 5)
    param = {"is_joint_torques": False, "is_external_wrench": True, "ts": TS}
    t0 = time.perf_counter()
    calculate_first_second_order_differentiation(model, q, param)
    dt = time.perf_counter() - t0
    per = dt / samples
    print("host path, human, %d samples: %.3f s = %.1f us per sample" % (samples, dt, 1e6 * per), flush=True)
    return {"model": "human", "samples": samples, "seconds": dt, "us_per_sample": 1e6 * per,
            "linear_extrapolation_seconds": {"1e6": per * 1e6, "1e7": per * 1e7},
            "note": "the unchanged host path (a Python loop over the samples around joint_difference), wall clock on this "
                    "machine's CPU; the figures for 1e6 and 1e7 samples are linear extrapolations, not measurements"}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-samples", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "differentiation.json"))
    args = ap.parse_args()
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("differentiation_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    _lib.profile_enable(True, 2)
    report = {"tool": "tools/differentiation_bench.py --repeats %d --baseline-samples %d" % (args.repeats, args.baseline_samples),
              "device": info["name"], "cu_count": info["cu_count"], "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
              "note": "device time of the library's own event pairs, one warm-up then the repeats; bytes = what the launch has "
                      "to move once (inputs read once, outputs written once)",
              "difference": [measure_difference("human", 10 ** 6, args.repeats), measure_difference("human", 10 ** 7, args.repeats),
                             measure_difference("ur10", 10 ** 6, args.repeats)],
              "medfilt": measure_medfilt(10 ** 6, 46, 5, args.repeats)}
    _lib.profile_enable(False)
    report["host_baseline"] = host_baseline(args.baseline_samples)
    report["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
