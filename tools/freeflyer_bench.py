#!/usr/bin/env python3
"""The free-flyer real-data entries -- quaternion logarithm, exponential with the sign test, wrench transport -- device time by
HIP events.

    freeflyer_bench.py [--repeats R] [--baseline-samples B] [--sizes 1000000,10000000] [--out profiles/freeflyer.json]

The human model (nq 46: a row of q is 368 bytes, the root free-flyer its first 7 doubles) at 1e6 and 1e7 samples:
(1) figh_quat_log of q[:, 3:7] (family "quat_log");
(2) figh_rotvec_to_quat against q[:, 3:7], written over columns 3:7 of a second q-like buffer, as filter_free_flyer does
    (family "rotvec_to_quat");
(3) figh_wrench_transport (family "wrench_transport"): the script's two uses -- se3ActionInverse of a sample-layout wrench into
    the stacked tau (examples/human/identification.py:434-453) and se3Action of a stacked wrench into a stacked one (:471-555).
Device time is that of the library's own event pairs (figh_profile_enable(2)), one warm-up, then R repeats.

BYTES are counted as the 128-byte lines a launch touches, not the values it uses: of a 368-byte row of q the kernels read 32
or 56 bytes, which is one or two lines -- the memory system moves the lines.  Dense arrays (rotation vectors, wrenches) count
their own size.  The fraction of the achievable HBM rate (6.3 TB/s on the MI355X) is bytes / time / rate.

The baseline is the reference's way of doing it: a Python loop over the samples (examples/human/identification.py:332-337,
:351-364, :436-453), here around the package's NumPy mirrors, at B samples (default 1e4) on this machine's CPU, and its LINEAR
EXTRAPOLATION to the sizes above, labelled as such.  The compiler's resource remarks of the translation unit are attached."""
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
from figaroh_plus_amd.identification import identification_tools as it  # noqa: E402
from figaroh_plus_amd.tools.randomdata import sample_inputs  # noqa: E402
from figaroh_plus_amd.tools.robot import Robot  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s
LINE = 128
BLOCK = 10 ** 6  # samples generated on the host; larger sets repeat this block on the device


def kernel_resources():
    csrc = os.path.join(ROOT, "figaroh_plus_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(csrc, "figh_freeflyer.hip"), "-o", os.devnull], capture_output=True, text=True)
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


def window_line_bytes(N, ld, first, width):
    """Bytes of the 128-byte lines that hold columns [first, first + width) of an N x ld array of doubles (base on a line
    boundary; the windows of two rows never share a line when 8 ld >= 8 width + 128)."""
    start = 8 * (np.arange(N, dtype=np.int64) * ld + first)
    last = start + 8 * width - 1
    lines = last // LINE - start // LINE + 1
    if 8 * ld < 8 * width + LINE:  # rows close together: count distinct lines
        lines = np.unique(np.concatenate([start // LINE, last // LINE])).size
        return int(lines) * LINE
    return int(lines.sum()) * LINE


def dense_line_bytes(count):
    return -(-8 * count // LINE) * LINE


def resident_positions(model, N):
    """N x nq device array: one host block of valid configurations, repeated on the device."""
    q, _, _ = sample_inputs(model, min(N, BLOCK), np.random.default_rng(0), 1.5, 2, 5)
    block = _lib.DeviceArray.from_host(np.ascontiguousarray(q).reshape(-1))
    if N <= BLOCK:
        return block
    d_q = _lib.DeviceArray((N * model.nq,), np.float64)
    lib = _lib.load()
    for lo in range(0, N, BLOCK):
        n = min(BLOCK, N - lo)
        _lib.check(lib.figh_memcpy_d2d(d_q.ptr + 8 * lo * model.nq, block.ptr, 8 * n * model.nq))
    return d_q


def resident_random(count, seed, scale):
    block = _lib.DeviceArray.from_host(np.random.default_rng(seed).uniform(-scale, scale, min(count, 6 * BLOCK)))
    if count <= block.size:
        return block
    d = _lib.DeviceArray((count,), np.float64)
    lib = _lib.load()
    for lo in range(0, count, block.size):
        _lib.check(lib.figh_memcpy_d2d(d.ptr + 8 * lo, block.ptr, 8 * min(block.size, count - lo)))
    return d


def timed(family, repeats, call):
    ms = []
    for k in range(repeats + 1):
        _lib.profile_reset()
        call()
        _lib.synchronize()
        if k:  # (k == 0: warm-up)
            ms.append(_lib.profile_get(family)[1])
    return ms


def entry(family, what, ms, nbytes, used):
    frac = [nbytes / HBM_ACHIEVABLE / (t * 1e-3) for t in ms]
    print("  %-58s %s ms, %.0f MB in lines (%.0f MB used), %.2f of the achievable rate"
          % (what, ["%.3f" % t for t in ms], nbytes / 1e6, used / 1e6, max(frac)), flush=True)
    return {"family": family, "what": what, "ms": ms, "line_bytes": nbytes, "value_bytes": used,
            "fraction_of_achievable_hbm": frac}


def measure(N, repeats):
    model = Robot.from_flat("human").model
    handle = _lib.ModelHandle(model.to_flat())
    nq = model.nq
    joint = model.getJointId("root_joint")
    print("human, N = %.0e" % N, flush=True)
    d_q = resident_positions(model, N)
    d_rv = _lib.DeviceArray((3 * N,), np.float64)
    quat_ptr = d_q.ptr + 8 * 3
    out = []
    ms = timed("quat_log", repeats, lambda: _lib.quat_log(quat_ptr, N, nq, d_rv.ptr, 3))
    out.append(entry("quat_log", "log: q[:, 3:7] (ld 46) -> rotvec (N, 3)", ms,
                     window_line_bytes(N, nq, 3, 4) + dense_line_bytes(3 * N), 8 * 7 * N))
    d_q2 = _lib.DeviceArray((N * nq,), np.float64)
    _lib.check(_lib.load().figh_memcpy_d2d(d_q2.ptr, d_q.ptr, 8 * N * nq))
    ms = timed("rotvec_to_quat", repeats, lambda: _lib.rotvec_to_quat(d_rv.ptr, N, 3, quat_ptr, nq, d_q2.ptr + 8 * 3, nq))
    # (the lines of the written window are counted once, as written: 32 of their 128 or 256 bytes change, and whatever the
    # memory system reads to merge them is not counted -- the fraction is a lower bound)
    out.append(entry("rotvec_to_quat", "exp: rotvec, q[:, 3:7] -> q_f[:, 3:7] (both ld 46)", ms,
                     dense_line_bytes(3 * N) + 2 * window_line_bytes(N, nq, 3, 4), 8 * 11 * N))
    d_q2.free()
    d_F, d_tau, d_w = resident_random(6 * N, 1, 100.0), _lib.DeviceArray((6 * N,), np.float64), _lib.DeviceArray((6 * N,), np.float64)
    q_lines = window_line_bytes(N, nq, model.joints[joint].idx_q, 7)
    ms = timed("wrench_transport", repeats,
               lambda: _lib.wrench_transport(handle, joint, N, d_q.ptr, nq, d_F.ptr, "sample", True, d_tau.ptr, "stacked"))
    out.append(entry("wrench_transport", "transport, inverse: sample (N, 6) -> stacked tau  [:434-453]", ms,
                     q_lines + 2 * dense_line_bytes(6 * N), 8 * 19 * N))
    ms = timed("wrench_transport", repeats,
               lambda: _lib.wrench_transport(handle, joint, N, d_q.ptr, nq, d_tau.ptr, "stacked", False, d_w.ptr, "stacked"))
    out.append(entry("wrench_transport", "transport, action: stacked -> stacked  [:471-555]", ms,
                     q_lines + 2 * dense_line_bytes(6 * N), 8 * 19 * N))
    ms = timed("wrench_transport", repeats,
               lambda: _lib.wrench_transport(handle, joint, N, d_q.ptr, nq, d_tau.ptr, "stacked", False, d_w.ptr, "sample"))
    out.append(entry("wrench_transport", "transport, action: stacked -> sample (N, 6)", ms,
                     q_lines + 2 * dense_line_bytes(6 * N), 8 * 19 * N))
    for d in (d_q, d_rv, d_F, d_tau, d_w):
        d.free()
    return {"model": "human", "samples": N, "nq": nq, "row_bytes": 8 * nq, "q_line_bytes_per_sample_transport": q_lines / N,
            "launches": out}


def host_baseline(samples, sizes):
    model = Robot.from_flat("human").model
    q, _, _ = sample_inputs(model, samples, np.random.default_rng(2), 1.5, 2, 5)
    F = np.random.default_rng(3).uniform(-100, 100, (samples, 6))
    t0 = time.perf_counter()
    rotvec = np.array([it.quaternion_log_mirror(q[ii, 3:7])[0] for ii in range(samples)])
    t1 = time.perf_counter()
    quat = np.zeros((samples, 4))
    for ii in range(samples):
        quat[ii] = it.rotation_vector_to_quaternion_mirror(rotvec[ii], q[ii, 3:7])[0]
    t2 = time.perf_counter()
    tau = np.empty(6 * samples)
    for ii in range(samples):
        tau[ii::samples] = it.transport_wrench_mirror(model, q[ii:ii + 1], F[ii:ii + 1], "root_joint", True, "sample", "stacked")
    t3 = time.perf_counter()
    out = {"samples": samples,
           "note": "a Python loop over the samples around the package's NumPy mirrors -- the shape of the reference's loops "
                   "around pin.log3 / pin.exp3 / se3ActionInverse -- wall clock on this machine's CPU; the figures for the "
                   "larger sizes are LINEAR EXTRAPOLATIONS, not measurements"}
    for name, dt in (("log", t1 - t0), ("exp", t2 - t1), ("transport", t3 - t2)):
        per = dt / samples
        print("host loop, %-9s %d samples: %.3f s = %.1f us per sample" % (name, samples, dt, 1e6 * per), flush=True)
        out[name] = {"seconds": dt, "us_per_sample": 1e6 * per,
                     "linear_extrapolation_seconds": {"%.0e" % n: per * n for n in sizes}}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-samples", type=int, default=10000)
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freeflyer.json"))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    _lib.load()
    if _lib.device_count() <= 0:
        sys.exit("freeflyer_bench.py measures on a HIP device; none found")
    info = _lib.device_info()
    _lib.profile_enable(True, 2)
    report = {"tool": "tools/freeflyer_bench.py --repeats %d --baseline-samples %d --sizes %s"
                      % (args.repeats, args.baseline_samples, args.sizes),
              "device": info["name"], "cu_count": info["cu_count"], "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
              "note": "device time of the library's own event pairs, one warm-up then the repeats; line_bytes = the 128-byte "
                      "lines the launch touches (a 368-byte row of q gives up 56 bytes, in one or two lines), value_bytes = "
                      "the values it uses; the fraction is line_bytes / time / achievable rate",
              "sizes": [measure(n, args.repeats) for n in sizes]}
    _lib.profile_enable(False)
    report["host_baseline"] = host_baseline(args.baseline_samples, sizes)
    report["kernel_resources"] = kernel_resources()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
