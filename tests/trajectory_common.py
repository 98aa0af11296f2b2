"""References for the excitation-trajectory tests (test_trajectory_host.py, test_trajectory_exact.py).

Two things, both written independently of the package's vectorised mirror (figaroh_plus_amd/tools/excitation.py):

* ``spline_emul``: the operation order of csrc/figh_trajectory.hip in scalar, loop form on Python floats (IEEE binary64, one
  correctly rounded operation per ``+ - * /``, no contraction).  The GPU tests assert ``np.array_equal`` with it.
* ``spline_exact``: the quintic in 50-digit arithmetic (mpmath) from the float64 inputs and the float64 sample times as given,
  with the error scale S of every entry: the sum of the absolute values of everything that is added.

C_SPLINE, from counting roundings (each contributes at most 2^-53 of a partial result bounded by S):
  - a coefficient: c5 is the longest.  h is a rounded difference and enters h5 five times (5) through four products (4); the
    numerator's middle term 6 * (v1 + v0) * h has the sum, the product by 6, h and the product by h (4); two subtractions
    join the terms (2) and one division ends it (1): 16, and 17 for c4 / c5's last terms counted the same way at their worst;
  - Horner: five products and five sums (10);
  - u = t - tps[k] is one rounding, and u^m carries it m <= 5 times (5).
  17 + 10 + 5 = 32 for q (30 for dq, 27 for ddq, whose factors k and k (k - 1) add one rounding each and whose powers of u are
  lower), to first order.  The count lands on a power of two; "the next power of two above the count" is taken literally, 64,
  which also covers the second-order terms.  32 itself would hold as well on every case of the suites (the largest ratio seen
  is below 3): the worst case of the count needs every rounding at its limit with one sign."""
import numpy as np

C_SPLINE = 64.0
# largest |emulation - exact| / (2^-53 S) seen over the cases of test_trajectory_host.py (HOST_CASES, gpu_shapes(), the
# 100-waypoint case): 2.73 (`unequal_one`)
EPS = 2.0 ** -53
SENTINEL = -7.25e77


# ------------------------------------------------------------------------------------------------------------ emulation
def sample_times(freq, tps, n_per=None):
    """(N, t, k, u-cap h) lists: t_i = tps[0] + i * (1 / freq), segment k_i, for i < n_per (default: the reference's N)."""
    tps = [float(x) for x in np.asarray(tps).reshape(-1)]
    delta_t = 1 / freq
    N = int((tps[-1] - tps[0]) / delta_t) + 1
    n = N if n_per is None else n_per
    t, seg = [], []
    for i in range(n):
        ti = tps[0] + i * delta_t
        k = 0
        while k + 1 <= len(tps) - 2 and tps[k + 1] <= ti:
            k += 1
        t.append(ti)
        seg.append(k)
    return N, t, seg


def segment_coefficients(h, p0, p1, v0, v1, a0, a1, plant=None):
    h2 = h * h
    h3 = h2 * h
    h4 = h3 * h
    h5 = h4 * h
    D = p1 - p0
    c3 = ((20.0 * D - (8.0 * v1 + 12.0 * v0) * h) - (3.0 * a0 - a1) * h2) / (2.0 * h3)
    c4 = ((-30.0 * D + ((16.0 if plant == "c4" else 14.0) * v1 + 16.0 * v0) * h) + (3.0 * a0 - 2.0 * a1) * h2) / (2.0 * h4)
    c5 = ((12.0 * D - (6.0 * (v1 + v0)) * h) - (a0 - a1) * h2) / (2.0 * h5)
    return (p0, v0, a0 / 2.0, c3, c4, c5)


def horner(c, u):
    c0, c1, c2, c3, c4, c5 = c
    q = ((((c5 * u + c4) * u + c3) * u + c2) * u + c1) * u + c0
    dq = ((((5.0 * c5) * u + 4.0 * c4) * u + 3.0 * c3) * u + 2.0 * c2) * u + c1
    ddq = (((20.0 * c5) * u + 12.0 * c4) * u + 6.0 * c3) * u + 2.0 * c2
    return q, dq, ddq


def spline_emul(freq, tps, wps, vel, acc, n_per=None, plant=None):
    """(t, q, dq, ddq): t (n,), the others (n, n_act), of ONE trajectory (wps, vel, acc: (n_act, n_wps)).
    ``plant``: "c4" (the 14 of c4 replaced by 16) or "segment" (a sample on a waypoint reads the coefficients of the segment
    before it)."""
    tps_l = [float(x) for x in np.asarray(tps).reshape(-1)]
    wps, vel, acc = (np.asarray(x, dtype=np.float64) for x in (wps, vel, acc))
    n_act, n_wps = wps.shape
    _, t, seg = sample_times(freq, tps_l, n_per)
    out = np.zeros((3, len(t), n_act))
    for s in range(n_act):
        coef = []
        for k in range(n_wps - 1):
            coef.append(segment_coefficients(tps_l[k + 1] - tps_l[k], float(wps[s, k]), float(wps[s, k + 1]), float(vel[s, k]),
                                             float(vel[s, k + 1]), float(acc[s, k]), float(acc[s, k + 1]), plant))
        for i, (ti, k) in enumerate(zip(t, seg)):
            u = ti - tps_l[k]
            h = tps_l[k + 1] - tps_l[k]
            if not u < h:
                u = h
            if plant == "segment" and k > 0 and ti == tps_l[k]:
                k -= 1  # (the local time of the right segment, the coefficients of the one before it)
            out[0, i, s], out[1, i, s], out[2, i, s] = horner(coef[k], u)
    return np.array(t), out[0], out[1], out[2]


def full_config_emul(q0, nv, act_idxq, act_idxv, q_act, dq_act, ddq_act):
    """The scatter of get_full_config (cubic_spline.py:171-178)."""
    n = len(q_act)
    q = np.array([np.asarray(q0, dtype=np.float64)] * n)
    v, a = np.zeros((n, nv)), np.zeros((n, nv))
    q[:, act_idxq] = q_act
    v[:, act_idxv] = dq_act
    a[:, act_idxv] = ddq_act
    return q, v, a


# ---------------------------------------------------------------------------------------------------------------- exact
def spline_exact(tps, wps, vel, acc, t):
    """(ref, S): object arrays (3, len(t), n_act) of 50-digit values and error scales of q, dq, ddq at the float64 times t."""
    import mpmath as mp
    mp.mp.dps = 50
    tp = [mp.mpf(float(x)) for x in np.asarray(tps).reshape(-1)]
    wps, vel, acc = (np.asarray(x, dtype=np.float64) for x in (wps, vel, acc))
    n_act, n_wps = wps.shape
    ref = np.empty((3, len(t), n_act), dtype=object)
    S = np.empty((3, len(t), n_act), dtype=object)
    for s in range(n_act):
        segs = []
        for k in range(n_wps - 1):
            h = tp[k + 1] - tp[k]
            p0, p1, v0, v1, a0, a1 = (mp.mpf(float(x)) for x in (wps[s, k], wps[s, k + 1], vel[s, k], vel[s, k + 1], acc[s, k],
                                                                   acc[s, k + 1]))
            D = p1 - p0
            c = [p0, v0, a0 / 2,
                 (20 * D - (8 * v1 + 12 * v0) * h - (3 * a0 - a1) * h ** 2) / (2 * h ** 3),
                 (-30 * D + (14 * v1 + 16 * v0) * h + (3 * a0 - 2 * a1) * h ** 2) / (2 * h ** 4),
                 (12 * D - 6 * (v1 + v0) * h - (a0 - a1) * h ** 2) / (2 * h ** 5)]
            A = abs(p0) + abs(p1)
            sc = [abs(p0), abs(v0), abs(a0) / 2,
                  (20 * A + (8 * abs(v1) + 12 * abs(v0)) * h + (3 * abs(a0) + abs(a1)) * h ** 2) / (2 * h ** 3),
                  (30 * A + (14 * abs(v1) + 16 * abs(v0)) * h + (3 * abs(a0) + 2 * abs(a1)) * h ** 2) / (2 * h ** 4),
                  (12 * A + 6 * (abs(v1) + abs(v0)) * h + (abs(a0) + abs(a1)) * h ** 2) / (2 * h ** 5)]
            segs.append((h, c, sc))
        for i, ti in enumerate(t):
            ti = mp.mpf(float(ti))
            k = 0
            while k + 1 <= n_wps - 2 and tp[k + 1] <= ti:
                k += 1
            h, c, sc = segs[k]
            u = min(ti - tp[k], h)
            for d, fac in enumerate(([1, 1, 1, 1, 1, 1], [0, 1, 2, 3, 4, 5], [0, 0, 2, 6, 12, 20])):
                ref[d, i, s] = sum(fac[m] * c[m] * u ** (m - d) for m in range(d, 6))
                S[d, i, s] = sum(fac[m] * sc[m] * u ** (m - d) for m in range(d, 6))
    return ref, S


def worst_ratio(got, ref, S):
    """max over entries of |got - ref| / (2^-53 S) (0 where S is 0 and the entry is exact)."""
    import mpmath as mp
    worst = 0.0
    for g, r, s in zip(np.asarray(got, dtype=np.float64).reshape(-1), ref.reshape(-1), S.reshape(-1)):
        err = abs(mp.mpf(float(g)) - r)
        if s == 0:
            assert err == 0
            continue
        worst = max(worst, float(err / (mp.mpf(EPS) * s)))
    return worst


# ---------------------------------------------------------------------------------------------------------------- cases
def waypoint_set(rng, n_act, n_wps, scale=1.0, zero_rates=False, B=None):
    shape = (n_act, n_wps) if B is None else (B, n_act, n_wps)
    wps = scale * rng.uniform(-1.5, 1.5, size=shape)
    if zero_rates:
        return wps, np.zeros(shape), np.zeros(shape)
    return wps, scale * rng.uniform(-2.0, 2.0, size=shape), scale * rng.uniform(-5.0, 5.0, size=shape)


# (tag, tps, freq): samples on interior waypoints, never on them, one segment, unequal segments
HOST_CASES = [
    ("one_segment", [0.0, 1.0], 16),
    ("on_waypoints", [0.0, 0.5, 1.0, 1.5], 8),
    ("freq7", [0.5 * i for i in range(5)], 7),
    ("unequal", [0.25, 0.6, 1.7, 1.95, 3.0], 10),
]

MODEL_CASES = {
    "ur10_all": ("ur10", ["shoulder_pan_joint", "shoulder_lift_joint", "elbow_joint", "wrist_1_joint", "wrist_2_joint",
                          "wrist_3_joint"]),
    "ur10_two": ("ur10", ["shoulder_pan_joint", "wrist_1_joint"]),
    "tiago_arm": ("tiago", ["torso_lift_joint", "arm_1_joint", "arm_2_joint", "arm_3_joint", "arm_4_joint", "arm_5_joint",
                            "arm_6_joint", "arm_7_joint"]),
    "human_arms": ("human", ["right_shoulder_Z", "right_shoulder_X", "right_shoulder_Y", "right_elbow_Z", "right_elbow_Y",
                             "left_shoulder_Z", "left_elbow_Z"]),
}


def model_case(name):
    """(robot, spline factory, q0 fill): the fill is not the neutral configuration (every inactive column is visible), and the
    human model's free-flyer keeps a unit quaternion."""
    from figaroh_plus_amd.tools.excitation import CubicSpline
    from figaroh_plus_amd.tools.robot import Robot
    model, joints = MODEL_CASES[name]
    robot = Robot.from_flat(model)
    rng = np.random.default_rng(len(name))
    q0 = robot.q0 + 0.0
    for j in robot.model.joints[1:]:
        if j.jtype in (0, 1):
            q0[j.idx_q] = rng.uniform(-1, 1)
        elif j.jtype == 2:
            ang = rng.uniform(-3, 3)
            q0[j.idx_q:j.idx_q + 2] = np.cos(ang), np.sin(ang)
        else:
            quat = rng.normal(size=4)
            q0[j.idx_q:j.idx_q + 3] = rng.uniform(-1, 1, size=3)
            q0[j.idx_q + 3:j.idx_q + 7] = quat / np.linalg.norm(quat)
    robot.q0 = q0
    return robot, (lambda n_wps: CubicSpline(robot, n_wps, joints)), q0


# raw-entry shapes of the GPU test: (tag, tps, freq, n_per, B, per-trajectory rates, scale).  n_per is given to the entry as
# it is: below the reference's N it is a prefix, above it the samples behind the last time point sit at the end of the last
# segment (the cap on u).
def gpu_shapes():
    rng = np.random.default_rng(77)
    unequal = np.cumsum(rng.uniform(0.2, 0.45, size=10))
    return [
        ("one_segment", [0.0, 1.0], 100, 2, 1, False, 1.0),
        ("one_segment_ragged", [0.25, 1.0], 64, 45, 3, True, 1.0),
        ("on_waypoints", [0.0, 0.5, 1.0], 64, 65, 3, True, 1.0),
        ("on_waypoints_big", [0.0, 0.5, 1.0], 64, 63, 3, False, 2.0 ** 20),
        ("freq7_past_the_end", [0.5 * i for i in range(10)], 7, 63, 3, True, 1.0),
        ("freq7_tiny", [0.5 * i for i in range(10)], 7, 32, 1, False, 2.0 ** -20),
        ("unequal", list(unequal), 100, 257, 3, True, 1.0),
        ("unequal_one", list(unequal), 100, 257, 1, False, 1.0),
    ]
