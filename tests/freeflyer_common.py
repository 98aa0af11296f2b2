"""Shared by test_freeflyer_host.py (CPU) and test_freeflyer_entrywise.py (GPU): the inputs of every regime and an EXACT
restatement of figh_quat_log, figh_rotvec_to_quat and figh_wrench_transport, written independently of the package's mirrors.

The restatement works in mpmath at 50 digits on the float64 inputs.  Every entry comes with its scale S -- the same formula on
absolute values, plus the conditioning of the one transcendental argument that carries roundings -- and the checks read
``|got - exact| <= C 2^-53 S``.  An entry with S = 0 must be a zero (of either sign: a negated representative carries -0.0).

* log.  r_k = sgn(w) (2 atan2(n, |w|) / n) x_k has no subtraction: S = |r_k|.  (atan2(n, |w|) moves by at most its own relative
  error when n and |w| move by theirs, so the roundings of n stay a multiple of u |r_k|.)
* exp.  theta = sqrt(sum of squares) carries two roundings, so theta / 2 moves by theta u.  cos(theta / 2) then moves by
  |sin(theta / 2)| theta u and sin(theta / 2) / theta by |cos(theta / 2)| u:  S_w = |cos(theta / 2)| + theta |sin(theta / 2)|,
  S_k = (|sin(theta / 2)| / theta + |cos(theta / 2)|) |r_k|  (theta = 0: S_w = 1, S_k = 0).  At theta = pi - 1e-6 the scalar
  part is 5e-7 and S_w = pi: what a float64 evaluation of cos near pi / 2 is worth.
* transport.  class ``V`` of kinematics_common: |A| |B| for every product, a sum of moduli for every sum, through the walk
  oM = prod placement_j M_j(q_j) (trigonometric leaves of scale |cos|, |sin|) and through the action.

C_ORACLE_* is the largest ratio of the package's float64 NumPy mirror against the restatement over exactly the rows of the
GPU suite (every regime and case below, N_REF rows; the smaller N of the suite are prefixes), measured on the CPU by
``python tests/freeflyer_common.py``; C_TOL_* is the power of two in [8, 16] x C_ORACLE_*, the project's rule for C_KIN and
C_PEE.  test_freeflyer_host.py::test_freeflyer_c_oracle_matches_the_recorded_figures recomputes them.
"""
import functools

import mpmath
import numpy as np

from differentiation_common import random_tree_model
from kinematics_common import IDENT, ONE, ZERO, V, hom_inv, hom_of_se3, joint_hom, mat_mul, vadd, vmul

mpmath.mp.dps = 50
mpf = mpmath.mpf
U = 2.0 ** -53
SENTINEL = -6.02214076e23

# measured on the CPU by measure_c_oracle() below (python tests/freeflyer_common.py)
C_ORACLE_LOG = 2.66956   # worst regime: see measure_c_oracle
C_ORACLE_EXP = 2.03425
C_ORACLE_TRN = 1.9736
C_TOL_LOG = 32.0   # power of two in [8, 16] x C_ORACLE_LOG
C_TOL_EXP = 32.0   # power of two in [8, 16] x C_ORACLE_EXP
C_TOL_TRN = 16.0   # power of two in [8, 16] x C_ORACLE_TRN

GPU_N = (1, 63, 64, 65, 257)
N_REF = 257
KEEP_ABOVE = 0.7071067811865476
MARGIN = 1e-9


def tol_rule(c_oracle):
    """The power of two in [8, 16] x c_oracle (the smallest power of two >= 8 c_oracle)."""
    return float(2.0 ** np.ceil(np.log2(8.0 * c_oracle)))


# ------------------------------------------------------------------------------------------------------------------- inputs
def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return v / np.linalg.norm(v, axis=1)[:, None]


LOG_REGIMES = ("n_0", "n_1e-12", "n_1e-7", "n_1e-3", "generic", "w_0", "w_pm1e-9", "w_negative", "non_unit")


@functools.lru_cache(maxsize=None)
def log_inputs(regime, n=N_REF):
    """(n, 4) quaternions (x y z w) of a regime of the logarithm.  2^-13 = 1.2e-4 is the series threshold: every regime is a
    factor of eight or more away from it."""
    rng = np.random.default_rng(100 + LOG_REGIMES.index(regime))
    sign = np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    if regime.startswith("n_"):
        nv = float(regime[2:])
        vec = _unit(rng, n, 3) * nv
        w = sign * np.sqrt(1.0 - nv * nv) if nv else sign * rng.uniform(0.5, 1.5, n)
        return np.c_[vec, w]
    if regime == "generic":
        return _unit(rng, n, 4)
    if regime == "w_0":
        return np.c_[_unit(rng, n, 3), np.zeros(n)]
    if regime == "w_pm1e-9":
        return np.c_[_unit(rng, n, 3), sign * 1e-9]
    if regime == "w_negative":
        q = _unit(rng, n, 4)
        q[:, 3] = -np.abs(q[:, 3])
        return q
    assert regime == "non_unit"
    return _unit(rng, n, 4) * (1.0 + sign * 1e-3)[:, None]


EXP_REGIMES = ("theta_0", "theta_1e-10", "generic_scalar_case", "generic_vector_case", "pi-1e-6", "beyond_pi")
REF_MODES = ("same", "below_-0.8", "abs_below_0.6", "generic")  # row i of a regime uses REF_MODES[i % 4]


def _float_canonical(r):
    """Eigen's representative of exp3(r) in float64 (input construction only: the references are built around it)."""
    th = np.linalg.norm(r, axis=1)
    with np.errstate(all="ignore"):
        a = np.where(th < 1e-6, 0.5, np.sin(0.5 * th) / th)
    q = np.c_[a[:, None] * r, np.cos(0.5 * th)]
    lead = np.where(np.abs(q[:, 3]) > 0.5, q[:, 3], q[np.arange(len(q)), np.argmax(np.abs(q[:, :3]), axis=1)])
    return q * np.where(lead < 0.0, -1.0, 1.0)[:, None]


@functools.lru_cache(maxsize=None)
def exp_inputs(regime, n=N_REF):
    """((n, 3) rotation vectors, (n, 4) reference quaternions).  generic_scalar_case: |cos(theta / 2)| > 1/2, Eigen makes w
    positive; generic_vector_case and pi-1e-6: the largest vector component positive; beyond_pi (filter overshoot): both,
    with a negative scalar part.  The references cycle through REF_MODES row by row: the canonical quaternion itself in
    float64 (d = 1 up to rounding, above 1 in some rows: these must keep), d < -0.8, |d| < 0.6, and d = cos(phi) for any phi
    that keeps d 1e-3 away from cos(pi / 4)."""
    k = EXP_REGIMES.index(regime)
    rng = np.random.default_rng(200 + k)
    ax = _unit(rng, n, 3)
    if regime == "theta_0":
        th = np.zeros(n)
    elif regime == "theta_1e-10":
        th = np.full(n, 1e-10)
    elif regime == "generic_scalar_case":
        th = rng.uniform(0.1, 1.9, n)          # 2 pi / 3 = 2.094: |cos(theta / 2)| = 1/2
    elif regime == "generic_vector_case":
        th = rng.uniform(2.3, 3.0, n)
    elif regime == "pi-1e-6":
        th = np.full(n, np.pi - 1e-6)
    else:
        th = rng.uniform(np.pi + 0.01, 5.5, n)
        near = np.abs(th - 4.0 * np.pi / 3.0) < 0.05  # 4 pi / 3: the other |cos(theta / 2)| = 1/2
        th[near] += 0.1
    r = ax * th[:, None]
    qE = _float_canonical(r)
    u = _unit(rng, n, 4)
    u -= np.sum(u * qE, axis=1)[:, None] * qE
    u /= np.linalg.norm(u, axis=1)[:, None]
    mode = np.arange(n) % 4
    d = np.ones(n)
    d[mode == 1] = rng.uniform(-0.99, -0.82, np.count_nonzero(mode == 1))
    d[mode == 2] = rng.uniform(-0.58, 0.58, np.count_nonzero(mode == 2))
    g = np.cos(rng.uniform(0.0, np.pi, np.count_nonzero(mode == 3)))
    g[np.abs(g - KEEP_ABOVE) < 1e-3] = 0.9
    d[mode == 3] = g
    ref = d[:, None] * qE + np.sqrt(np.maximum(1.0 - d * d, 0.0))[:, None] * u
    ref[mode == 0] = qE[mode == 0]
    ref[(mode == 0) & (np.arange(n) % 8 == 4)] *= 1.0 + 2.0 ** -50  # ... and a reference whose norm exceeds 1 by rounding
    return r, ref


def configurations(model, n, seed):
    """n configurations: revolute / prismatic in [-3, 3], continuous as (cos, sin), free-flyer position in [-1, 1]^3 with a
    uniform unit quaternion."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n, model.nq))
    for jm in model.joints[1:]:
        iq = jm.idx_q
        if jm.jtype == 2:
            ang = rng.uniform(-np.pi, np.pi, n)
            q[:, iq], q[:, iq + 1] = np.cos(ang), np.sin(ang)
        elif jm.jtype == 3:
            q[:, iq:iq + 3] = rng.uniform(-1, 1, (n, 3))
            q[:, iq + 3:iq + 7] = _unit(rng, n, 4)
        else:
            q[:, iq] = rng.uniform(-3.0, 3.0, n)
    return q


def mocap_like(model, n, seed):
    """A smooth trajectory: the free-flyer spins, the other joints swing."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)
    q = np.zeros((n, model.nq))
    for jm in model.joints[1:]:
        iq = jm.idx_q
        if jm.jtype == 3:
            q[:, iq:iq + 3] = rng.uniform(-1, 1, 3) + 0.1 * np.sin(2 * np.pi * t)[:, None] * rng.uniform(-1, 1, 3)
            ax = rng.standard_normal(3)
            ax /= np.linalg.norm(ax)
            # 8 rad/s at ts = 0.01: crosses theta = pi (w changes sign, the vector jumps), and 25 rows are 2 rad apart
            ang = 0.5 + 0.08 * np.arange(n) + 0.01 * rng.standard_normal(n)
            q[:, iq + 3:iq + 6] = np.sin(ang / 2)[:, None] * ax
            q[:, iq + 6] = np.cos(ang / 2)
        elif jm.jtype == 2:
            ang = rng.uniform(-1, 1) + 0.5 * np.sin(2 * np.pi * t)
            q[:, iq], q[:, iq + 1] = np.cos(ang), np.sin(ang)
        else:
            q[:, iq] = rng.uniform(-1, 1) + 0.3 * np.sin(2 * np.pi * t * rng.uniform(0.5, 2)) + 0.002 * rng.standard_normal(n)
    return q


def _placed_tree():
    """random_tree_model with placements that are not the identity (its own are): on the plain tree a placement on the wrong
    side, and p x f on the path r1 -> r5 (p = 0), cannot be told from the right statement."""
    from figaroh_plus_amd.model import SE3, rpy_to_matrix

    m = random_tree_model()
    for j in range(1, m.njoints):
        rng = np.random.default_rng(40 + j)
        m.jointPlacements[j] = SE3(rpy_to_matrix(*rng.uniform(-1.0, 1.0, 3)), rng.uniform(-0.2, 0.2, 3))
    return m


# name -> (model factory, joint): the human model with the free-flyer at joint 1; random_tree_model() with joint = its
# free-flyer (joint 3, behind a revolute and a continuous joint) and joint = its last joint; the same two with placements
TRANSPORT_CASES = ("human_root", "tree_freeflyer", "tree_last", "placed_tree_freeflyer", "placed_tree_last")


@functools.lru_cache(maxsize=None)
def transport_case(name):
    """(model, joint id)."""
    if name == "human_root":
        from figaroh_plus_amd.tools.robot import Robot

        m = Robot.from_flat("human").model
        assert m.getJointId("root_joint") == 1 and m.joints[1].jtype == 3
        return m, 1
    m = _placed_tree() if name.startswith("placed") else random_tree_model()
    j = 3 if name.endswith("freeflyer") else m.njoints - 1
    assert m.joints[3].jtype == 3 and [m.joints[k].jtype for k in (1, 2)] == [0, 2]
    return m, j


@functools.lru_cache(maxsize=None)
def transport_inputs(name, n=N_REF):
    """(q (n, nq), wrench (n, 6) in the sample layout): forces of order 100 N, moments of order 30 N m."""
    model, _ = transport_case(name)
    rng = np.random.default_rng(300 + TRANSPORT_CASES.index(name))
    F = np.c_[rng.uniform(-100, 100, (n, 3)), rng.uniform(-30, 30, (n, 3))]
    return configurations(model, n, 310 + TRANSPORT_CASES.index(name)), F


def to_layout(F, layout):
    """(N, 6) -> the array of ``layout``."""
    return np.ascontiguousarray(F) if layout == "sample" else np.ascontiguousarray(F.T).reshape(-1)


def from_layout(x, N, layout):
    x = np.asarray(x)
    return x.reshape(N, 6) if layout == "sample" else x.reshape(6, N).T


# -------------------------------------------------------------------------------------------------------- the restatement
LOG_PLANTS = ("wxyz", "no_sign")
EXP_PLANTS = ("wxyz",)
TRANSPORT_PLANTS = ("wxyz", "moment_first", "cross_before_rotation", "iMo", "placement_right")


class Exact:
    """Exact values (mpf object array), their float64 roundings with what the rounding dropped, and the scales."""

    def __init__(self, hi, scale, **info):
        self.hi, self.scale = hi, np.asarray(scale, dtype=np.float64)
        self.val = np.array(hi, dtype=np.float64)
        self.low = np.array(hi - self.val, dtype=np.float64)
        self.info = info

    def rows(self, n):
        return Exact(self.hi[:n], self.scale[:n], **{k: v[:n] for k, v in self.info.items()})

    def row(self, i):
        return Exact(self.hi[i:i + 1], self.scale[i:i + 1])


def ratio(got, ex):
    """(largest |got - exact| / (2^-53 S) over the entries with S > 0, whether every entry with S = 0 is a zero)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ex.val.shape, (got.shape, ex.val.shape)
    zero = ex.scale == 0.0
    zeros_ok = bool(np.all(got[zero] == 0.0))
    if np.all(zero):
        return 0.0, zeros_ok
    err = np.abs((got - ex.val) - ex.low)  # got - val is exact when they are within a factor of two (Sterbenz)
    return float(np.max(err[~zero] / (U * ex.scale[~zero]))), zeros_ok


def exact_log(quat, plant=None):
    hi = np.empty((len(quat), 3), dtype=object)
    S = np.zeros((len(quat), 3))
    for i, row in enumerate(quat):
        x, y, z, w = (mpf(float(t)) for t in (row[[1, 2, 3, 0]] if plant == "wxyz" else row))
        n = mpmath.sqrt(x * x + y * y + z * z)
        if n == 0:
            hi[i] = [mpf(0)] * 3
            continue
        f = 2 * mpmath.atan2(n, abs(w)) / n
        if w < 0 and plant != "no_sign":
            f = -f
        hi[i] = [f * x, f * y, f * z]
        S[i] = [abs(float(t)) for t in hi[i]]
    return Exact(hi, S)


def exact_exp(rotvec, ref, plant=None):
    """Exact figh_rotvec_to_quat; info: d (float), tie (float): the distance of the sample from Eigen's ties (|w^| = 1/2, and,
    in the vector case, the gap between the two largest vector components)."""
    n = len(rotvec)
    hi = np.empty((n, 4), dtype=object)
    S = np.zeros((n, 4))
    ds, ties, vector_case = np.zeros(n), np.zeros(n), np.zeros(n, dtype=bool)
    keep_above = mpf(KEEP_ABOVE)
    for i in range(n):
        r = [mpf(float(t)) for t in rotvec[i]]
        f = [mpf(float(t)) for t in (ref[i][[1, 2, 3, 0]] if plant == "wxyz" else ref[i])]
        th = mpmath.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        if th == 0:
            a, c, sa, sc = mpf(0.5), mpf(1), 1.5, 1.0
        else:
            sh, c = mpmath.sin(th / 2), mpmath.cos(th / 2)
            a = sh / th
            sa = abs(float(a)) + abs(float(c))
            sc = abs(float(c)) + float(th) * abs(float(sh))
        q = [a * r[0], a * r[1], a * r[2], c]
        if abs(c) > mpf(0.5):
            lead = c
            ties[i] = abs(float(abs(c) - mpf(0.5)))
        else:
            mags = [abs(t) for t in q[:3]]
            k = 0
            if mags[1] > mags[k]:
                k = 1
            if mags[2] > mags[k]:
                k = 2
            lead = q[k]
            rest = sorted(mags)
            ties[i] = min(abs(float(abs(c) - mpf(0.5))), float(rest[2] - rest[1]))
            vector_case[i] = True
        sE = -1 if lead < 0 else 1
        d = sE * (q[0] * f[0] + q[1] * f[1] + q[2] * f[2] + q[3] * f[3])
        sg = sE if d > keep_above else -sE
        ds[i] = float(d)
        out = [sg * t for t in q]
        hi[i] = [out[3], out[0], out[1], out[2]] if plant == "wxyz" else out
        sc4 = [sa * abs(float(t)) for t in r] + [sc]
        S[i] = [sc4[3], sc4[0], sc4[1], sc4[2]] if plant == "wxyz" else sc4
    return Exact(hi, S, d=ds, tie=ties, vector_case=vector_case)


def _world_placement(model, q, joint, placement_right=False):
    """oMi[joint] at one configuration, a 4 x 4 of V: the product over the support path, root first."""
    path, j = [], int(joint)
    while j > 0:
        path.append(j)
        j = model.parents[j]
    M = IDENT
    for j in path[::-1]:
        pl, mj = hom_of_se3(model.jointPlacements[j]), joint_hom(model.joints[j], q)
        M = mat_mul(M, mat_mul(mj, pl) if placement_right else mat_mul(pl, mj))
    return M


def _vec(values):
    return [V(float(t)) if t != 0.0 else ZERO for t in values]


def _cross(a, b):
    return [vadd(vmul(a[1], b[2]), -vmul(a[2], b[1])), vadd(vmul(a[2], b[0]), -vmul(a[0], b[2])),
            vadd(vmul(a[0], b[1]), -vmul(a[1], b[0]))]


def _dot3(a, b):
    acc = ZERO
    for k in range(3):
        acc = vadd(acc, vmul(a[k], b[k]))
    return acc


def _apply(R, x, transpose=False):
    """R x (R^T x) for a 3 x 3 of V."""
    return [_dot3([R[k][r] if transpose else R[r][k] for k in range(3)], x) for r in range(3)]


def exact_transport(name, inverse, plant=None, n=N_REF):
    """Exact figh_wrench_transport of a case over its first n inputs, (n, 6) in the sample layout."""
    model, joint = transport_case(name)
    q, F = transport_inputs(name)
    hi = np.empty((n, 6), dtype=object)
    S = np.zeros((n, 6))
    for i in range(n):
        qi = q[i].copy()
        if plant == "wxyz":
            for jm in model.joints[1:]:
                if jm.jtype == 3:
                    qi[jm.idx_q + 3:jm.idx_q + 7] = q[i][jm.idx_q + 3:jm.idx_q + 7][[1, 2, 3, 0]]
        M = _world_placement(model, qi, joint, plant == "placement_right")
        if plant == "iMo":
            M = hom_inv(M)
        R = [[M[r][c] for c in range(3)] for r in range(3)]
        p = [M[r][3] for r in range(3)]
        w = _vec(F[i])
        f, m = (w[3:], w[:3]) if plant == "moment_first" else (w[:3], w[3:])
        if inverse:
            c = _cross(p, f)
            fo = _apply(R, f, transpose=True)
            mo = _apply(R, [vadd(m[d], -c[d]) for d in range(3)], transpose=True)
        else:
            fo = _apply(R, f)
            c = _cross(p, f if plant == "cross_before_rotation" else fo)
            rm = _apply(R, m)
            mo = [vadd(rm[d], c[d]) for d in range(3)]
        out = (mo + fo) if plant == "moment_first" else (fo + mo)
        hi[i] = [t.v for t in out]
        S[i] = [t.s for t in out]
    return Exact(hi, S)


@functools.lru_cache(maxsize=None)
def log_reference(regime):
    return exact_log(log_inputs(regime))


@functools.lru_cache(maxsize=None)
def exp_reference(regime):
    return exact_exp(*exp_inputs(regime))


@functools.lru_cache(maxsize=None)
def transport_reference(name, inverse):
    return exact_transport(name, inverse)


def measure_c_oracle():
    """(C_ORACLE_LOG, C_ORACLE_EXP, C_ORACLE_TRN): the mirrors against the restatement over every row of the GPU suite."""
    from figaroh_plus_amd.identification import identification_tools as it

    c_log = max(ratio(it.quaternion_log_mirror(log_inputs(r)), log_reference(r))[0] for r in LOG_REGIMES)
    c_exp = max(ratio(it.rotation_vector_to_quaternion_mirror(*exp_inputs(r)), exp_reference(r))[0] for r in EXP_REGIMES)
    c_trn = 0.0
    for name in TRANSPORT_CASES:
        model, joint = transport_case(name)
        q, F = transport_inputs(name)
        for inverse in (False, True):
            got = it.transport_wrench_mirror(model, q, F, joint, inverse, "sample", "sample")
            c_trn = max(c_trn, ratio(got, transport_reference(name, inverse))[0])
    return c_log, c_exp, c_trn


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("C_ORACLE_LOG %.6g  C_ORACLE_EXP %.6g  C_ORACLE_TRN %.6g" % measure_c_oracle())
