"""HIP-backed mirror of the LS / WLS / sigma helpers of
``src/figaroh/identification/identification_tools.py`` (:23-83, :168-331) plus the
least-squares statements that live inline in the example scripts.

Every pass over the tall matrices (residuals, weighted normal equations, covariance) is a
TSQR / block-norm kernel call; what remains on the host is O(r^2) algebra on the triangle.
"""
import operator

import numpy as np

from .. import _lib
from .._host import host_tail, relative_percent
from ..device import GpuMatrix, to_device, vector_to_device
from ..tools.qrdecomposition import rfactor


def get_param_from_yaml(robot, identif_data):
    """Flatten the YAML ``identification`` section into the ``param`` dict (identification_tools.py:23-83)."""
    rp = identif_data["robot_params"][0]
    pb = identif_data["problem_params"][0]
    pr = identif_data["processing_params"][0]
    tls = identif_data["tls_params"][0]
    param = {"robot_name": robot.model.name, "nb_samples": int(1 / (pr["ts"]))}
    for key in ("q_lim_def", "dq_lim_def", "fv", "fs", "Ia", "Iam6", "fvm6", "fsm6", "N", "ratio_essential"):
        param[key] = rp[key]
    param["off"] = rp["offset"]
    for key in ("is_external_wrench", "is_joint_torques", "force_torque", "external_wrench_offsets", "has_friction",
                "has_actuator_inertia", "has_joint_offset", "has_coupled_wrist"):
        param[key] = pb[key]
    param["cut_off_frequency_butterworth"] = pr["cut_off_frequency_butterworth"]
    param["ts"] = pr["ts"]
    param["mass_load"] = tls["mass_load"]
    param["which_body_loaded"] = tls["which_body_loaded"]
    return param


def set_missing_params_setting(robot, params_settings):
    """Defaults for what the URDF does not specify (identification_tools.py:86-165), statement for statement -- including
    the reference's own slips, which a drop-in keeps: ``diff_limit.any`` is never called (so the position limits are
    never replaced), the effort-limit branch tests the VELOCITY limits again and writes ``-tau_lim_def``, and the loops
    run over ``nq``.  Side effects on ``robot.model`` as in the reference; returns the updated ``params_settings``
    (``accelerationLimit``, ``fv`` / ``fs`` = (i + 1) / 10 with friction, ``OFFX`` / ``OFFY`` / ``OFFZ`` = 900 / 450 / 0
    with external-wrench offsets)."""
    model = robot.model
    diff_limit = np.setdiff1d(model.lowerPositionLimit, model.upperPositionLimit)
    if not diff_limit.any:  # (a bound method: always true, as in the reference)
        print("No joint limits. Set default values")
        for ii in range(model.nq):
            model.lowerPositionLimit[ii] = -params_settings["q_lim_def"]
            model.upperPositionLimit[ii] = params_settings["q_lim_def"]
    if np.sum(model.velocityLimit) == 0:
        print("No velocity limit. Set default value")
        for ii in range(model.nq):
            model.velocityLimit[ii] = params_settings["dq_lim_def"]
    if np.sum(model.velocityLimit) == 0:
        print("No joint torque limit. Set default value")
        for ii in range(model.nq):
            model.effortLimit[ii] = -params_settings["tau_lim_def"]
    accelerationLimit = np.zeros(model.nq)
    for ii in range(model.nq):
        accelerationLimit[ii] = params_settings["ddq_lim_def"]
    params_settings["accelerationLimit"] = accelerationLimit
    if params_settings["has_friction"]:
        params_settings["fv"] = [(ii + 1) / 10 for ii in range(model.nv)]
        params_settings["fs"] = [(ii + 1) / 10 for ii in range(model.nv)]
    if params_settings["external_wrench_offsets"]:
        params_settings["OFFX"] = 900
        params_settings["OFFY"] = 450
        params_settings["OFFZ"] = 0
    return params_settings


def base_param_from_standard(phi_standard, params_base):
    """Evaluate the regrouping expressions on standard-parameter values (identification_tools.py:168-201)."""
    ops = {"+": operator.add, "-": operator.sub}
    phi_base = []
    for expr in params_base:
        values, pending = [], []
        for tok in expr.split(" "):
            parts = tok.split("*")
            if len(parts) == 2:
                values.append(float(parts[0]) * phi_standard[parts[1]])
            elif parts[0] in ops:
                pending.append(ops[parts[0]])
            else:
                values.append(phi_standard[parts[0]])
        acc = values[0]
        for k, op in enumerate(pending):
            acc = op(acc, values[k + 1])
        phi_base.append(acc)
    return phi_base


def index_in_base_params(params, id_segments):
    """Map segment ids to the base parameters that contain them (identification_tools.py:237-288)."""
    names = ("Ixx", "Ixy", "Ixz", "Iyy", "Iyz", "Izz", "mx", "my", "mz", "m")
    hits = set()
    for seg in id_segments:
        wanted = {k + str(seg) for k in names}
        for ii, expr in enumerate(params):
            for tok in expr.split(" "):
                if any(p in wanted for p in tok.split("*")):
                    hits.add((seg, ii))
    grouped = {}
    for seg, ii in sorted(hits):
        grouped.setdefault(seg, []).append(ii)
    return dict(zip(range(len(id_segments)), grouped.values()))


def _triangle_with_tau(W_b, tau, block_weight=None):
    Raug = rfactor(W_b, tau=tau, block_weight=block_weight)
    r = Raug.shape[0] - 1
    return Raug[:r, :r], Raug[:r, r], Raug[r, r]


@host_tail
def least_squares(W_b, tau):
    """OLS solution of ``W_b phi = tau`` -- replaces ``np.linalg.pinv(W_base) @ tau``
    (examples/ur10/identification.py:159, examples/human/identification.py:467) and
    ``np.linalg.lstsq(W_b, tau)`` (examples/staubli_TX40/identification.py:240) for full-rank W_b."""
    R, z, _ = _triangle_with_tau(W_b, tau)
    return np.linalg.solve(R, z)


@host_tail
def relative_stdev(W_b, phi_b, tau):
    """Relative standard deviation (%) of the identified parameters (identification_tools.py:204-234).

    ||tau - W phi||^2 = ||R phi - Q^T tau||^2 + rho^2 and inv(W^T W) = R^-1 R^-T, both from one TSQR.
    """
    Wd, _ = to_device(W_b)
    phi_b = np.asarray(phi_b, dtype=np.float64)
    R, z, rho = _triangle_with_tau(Wd, tau)
    res2 = float(np.sum((R @ phi_b - z) ** 2) + rho ** 2)
    sig_ro_sqr = res2 / (Wd.rows - phi_b.shape[0])
    R_inv = np.linalg.inv(R)
    C_x = sig_ro_sqr * (R_inv @ R_inv.T)
    std_x_sqr = np.diag(C_x)
    return relative_percent(np.sqrt(std_x_sqr), phi_b)  # (an estimate of exactly zero: inf, like the reference's division)


def relative_stdev_from_normal_terms(G, g, tau_sq, rows, phi_b):
    """``relative_stdev`` (identification_tools.py:204-234) from the normal-equation terms of the base regressor -- G = W_b^T
    W_b, g = W_b^T tau, tau^T tau, row count -- as ``dist.allreduce_normal_terms`` sums them over sample shards:
    ||tau - W_b phi||^2 = tau^T tau - 2 phi^T g + phi^T G phi, C = sigma^2 G^-1.  For well-conditioned base regressors (the
    difference of large numbers loses cond(W_b)^2 eps of the residual; the triangle form of :func:`relative_stdev` does
    not)."""
    phi_b = np.asarray(phi_b, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    res2 = float(tau_sq - 2.0 * phi_b @ g + phi_b @ G @ phi_b)
    sig_ro_sqr = res2 / (rows - phi_b.shape[0])
    C_x = sig_ro_sqr * np.linalg.inv(G)
    return relative_percent(np.sqrt(np.diag(C_x)), phi_b)


def block_residual_sqnorms(tau_meas, tau_est, nblocks):
    """Per-joint squared residual norms ||tau_j - tau_est_j||^2 on the device.  ``nblocks``: a number of
    equal blocks, or the list of block lengths (joints keep different numbers of rows after the zero-velocity
    rejection, examples/staubli_TX40/identification.py:207-233)."""
    d_a, d_b = vector_to_device(tau_meas), vector_to_device(tau_est)
    if np.isscalar(nblocks):
        out = _lib.DeviceArray((int(nblocks),), np.float64)
        _lib.block_sqnorm(d_a, d_b, d_a.size, int(nblocks), out)
        return out.to_host()
    res, off = [], 0
    one = _lib.DeviceArray((1,), np.float64)

    class _At:
        def __init__(self, base, k):
            self.ptr = base.ptr + 8 * k

    for n_i in nblocks:
        _lib.block_sqnorm(_At(d_a, off), _At(d_b, off), int(n_i), 1, one)
        res.append(float(one.to_host()[0]))
        off += int(n_i)
    return np.array(res)


@host_tail
def weigthed_least_squares(robot, phi_b, W_b, tau_meas, tau_est, param):
    """Library WLS (identification_tools.py:291-331), including its conventions: per-joint
    ``sigma_j = ||tau_j - tau_est_j|| / (n_j - len(phi_b))`` (a norm, not a variance), rows scaled by
    ``1/sigma_j``, ``phi = pinv(P W) P tau`` with all joints weighted, rounded to 6 decimals."""
    nq = robot.model.nq
    stops = [int(s) for s in param["idx_tau_stop"]][:nq]
    nb = stops[0]
    if stops != [nb * (k + 1) for k in range(nq)]:
        raise ValueError("weigthed_least_squares: idx_tau_stop must describe equal-length joint blocks "
                         "(the reference's P index jj + ii*nb_samples assumes it, identification_tools.py:319-321)")
    Wd, _ = to_device(W_b)
    tau_meas = np.ascontiguousarray(tau_meas, dtype=np.float64)
    if Wd.rows != nb * nq or tau_meas.shape[0] != Wd.rows:
        raise ValueError("W_b / tau_meas do not match idx_tau_stop")
    sq = block_residual_sqnorms(tau_meas, tau_est, nq)
    sigma = np.sqrt(sq) / (nb - len(phi_b))
    R, z, _ = _triangle_with_tau(Wd, tau_meas, block_weight=1.0 / sigma)
    return np.around(np.linalg.solve(R, z), 6)


@host_tail
def weighted_least_squares_blocks(W_b, tau, phi_b, nblocks, return_details=False):
    """Script WLS of examples/staubli_TX40/identification.py:305-346.  ``nblocks``: number of equal joint blocks or
    the list of block lengths.  sigma_j^2 = ||tau_j - W_j phi_b||^2 / n_j, phi = (W^T S^-1 W)^-1 W^T S^-1 tau
    (6 decimals), C_X = (W^T S^-1 W)^-1, std% = 100 sqrt(diag C_X) / |phi| (2 decimals).  Returns (phi, std%)."""
    Wd, _ = to_device(W_b)
    phi_b = np.ascontiguousarray(phi_b, dtype=np.float64)
    d_est = _lib.DeviceArray((Wd.rows,), np.float64)
    _lib.matvec(Wd.buf, Wd.rows, Wd.ld, None, Wd.cols, vector_to_device(phi_b), d_est)
    sq = block_residual_sqnorms(tau, d_est, nblocks)
    if np.isscalar(nblocks):
        sig2 = sq / (Wd.rows // int(nblocks))
        weights = 1.0 / np.sqrt(sig2)
    else:
        counts = np.asarray(nblocks, dtype=np.int64)
        weights = np.repeat(1.0 / np.sqrt(sq / counts), counts)  # one weight per row
    R, z, _rho = _triangle_with_tau(Wd, tau, block_weight=weights)
    phi = np.around(np.linalg.solve(R, z), 6)
    R_inv = np.linalg.inv(R)
    C_X = R_inv @ R_inv.T
    std = relative_percent(np.sqrt(np.diag(C_X)), phi)
    if return_details:  # the per-joint variances and the weighted triangle of [W_b tau]: what essential_parameters takes
        if np.isscalar(nblocks):
            sig2_joint = sq / (Wd.rows // int(nblocks))
        else:
            sig2_joint = sq / np.asarray(nblocks, dtype=np.float64)
        k = R.shape[0]
        Raug = np.zeros((k + 1, k + 1))
        Raug[:k, :k], Raug[:k, k], Raug[k, k] = R, z, _rho
        return phi, std, {"sigma2_joint": sig2_joint, "R_wls": Raug}
    return phi, std


# ----------------------------------------------------------------------------------------------------------
# Pre-processing on either side of the hot path ("next" row): finite differences and row
# rejection are O(N nq) NumPy statements as in the reference; the filters run on the device (figh_filtfilt_cols below).
def _quat_to_rot(x, y, z, w):
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _log3(R):
    tr = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    theta = np.arccos(tr)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if theta < 1e-8:
        return 0.5 * w
    if np.pi - theta < 1e-6:
        A = (R + np.eye(3)) / 2.0
        k = int(np.argmax(np.diag(A)))
        ax = A[:, k] / np.sqrt(A[k, k])
        return theta * (ax if w @ ax >= 0 else -ax)
    return theta / (2.0 * np.sin(theta)) * w


def _log6(R, p):
    """SE(3) logarithm, (linear, angular): w = log3(R), v = alpha p - w x p / 2 + beta (w . p) w."""
    w = _log3(R)
    t = np.linalg.norm(w)
    if t < 1e-4:
        alpha, beta = 1.0 - t * t / 12.0 - t ** 4 / 720.0, 1.0 / 12.0 + t * t / 720.0
    else:
        st, ct = np.sin(t), np.cos(t)
        alpha, beta = t * st / (2.0 * (1.0 - ct)), 1.0 / (t * t) - st / (2.0 * t * (1.0 - ct))
    return alpha * p - 0.5 * np.cross(w, p) + beta * (w @ p) * w, w


def joint_difference(model, q0, q1):
    """``pin.difference(model, q0, q1)`` (identification_tools.py:370,376) for the joint types of the URDF loader: the
    tangent vector from q0 to q1 -- q1 - q0 for revolute / prismatic joints, the angle of R0^T R1 for continuous ones
    (cos, sin), log6(M0^-1 M1) in the local frame for a free-flyer (linear, angular)."""
    out = np.zeros(model.nv)
    for j in model.joints[1:]:
        if j.jtype in (0, 1):
            out[j.idx_v] = q1[j.idx_q] - q0[j.idx_q]
        elif j.jtype == 2:  # (cos, sin): angle of R0^T R1
            c0, s0, c1, s1 = q0[j.idx_q], q0[j.idx_q + 1], q1[j.idx_q], q1[j.idx_q + 1]
            out[j.idx_v] = np.arctan2(s1 * c0 - c1 * s0, c1 * c0 + s1 * s0)
        else:  # free-flyer: q = [p, qx qy qz qw]
            iq, iv = j.idx_q, j.idx_v
            R0, R1 = _quat_to_rot(*q0[iq + 3:iq + 7]), _quat_to_rot(*q1[iq + 3:iq + 7])
            v, w = _log6(R0.T @ R1, R0.T @ (np.asarray(q1[iq:iq + 3]) - np.asarray(q0[iq:iq + 3])))
            out[iv:iv + 3], out[iv + 3:iv + 6] = v, w
    return out


def calculate_first_second_order_differentiation(model, q, param, dt=None):
    """(q, dq, ddq) by finite differences -- identification_tools.py:334-387, including its conventions: forward
    difference for dq, ``np.gradient`` of dq for ddq on joints ``range(model.nq - 1)`` only (the last joint's
    acceleration stays 0 for fixed-base robots), two samples dropped from q and one from dq / ddq.

    A ``GpuMatrix`` q, or ``param["device_resident"]``, takes the device path (figh_joint_difference +
    figh_gradient_cols): three ``GpuMatrix`` come back, prefixes of their buffers, ready for ``build_regressor_basic`` /
    ``IdentificationPipeline.set_samples`` without a copy."""
    if isinstance(q, GpuMatrix) or param.get("device_resident"):
        return _differentiate_device(model, q, param, dt)
    q = np.asarray(q, dtype=np.float64)
    ncol = q.shape[1] if param["is_joint_torques"] else q.shape[1] - 1
    if param["is_external_wrench"]:
        ncol = q.shape[1] - 1
    dq = np.zeros([q.shape[0] - 1, ncol])
    ddq = np.zeros([q.shape[0] - 1, ncol])
    only_simple = all(j.jtype in (0, 1) for j in model.joints[1:])
    if only_simple and model.nq == model.nv == ncol:
        step = np.diff(q, axis=0)
        dq[:, :] = step / (param["ts"] if dt is None else np.asarray(dt)[:len(step), None])
    else:
        for ii in range(q.shape[0] - 1):
            dq[ii, :] = joint_difference(model, q[ii, :], q[ii + 1, :]) / (param["ts"] if dt is None else dt[ii])
    h = param["ts"] if dt is None else dt
    for jj in range(model.nq - 1):
        ddq[:, jj] = np.gradient(dq[:, jj], edge_order=1) / h
    return q[:-2], dq[:-1], ddq[:-1]


def _divisor_to_device(h, count, what):
    """(scalar, device address or None, keep-alive) of a divisor that is a number or one value per row."""
    if isinstance(h, _lib.DeviceArray) or hasattr(h, "ptr"):
        if getattr(h, "size", count) != count:
            raise ValueError("%s must have %d entries, got %d" % (what, count, h.size))
        return 0.0, h.ptr, h
    if np.ndim(h) == 0:
        return float(h), None, None
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1)
    if h.shape[0] != count:
        raise ValueError("%s must have %d entries, got %d" % (what, count, h.shape[0]))
    d_h = _lib.DeviceArray.from_host(h)
    return 0.0, d_h.ptr, d_h


def _differentiate_device(model, q, param, dt):
    """calculate_first_second_order_differentiation with q, dq and ddq resident: dq = difference(q[i], q[i + 1]) / ts for
    every joint type (identification_tools.py:366-376), ddq = np.gradient(dq) / ts on the columns ``range(model.nq - 1)``
    (:378-384), ``dt`` per pair for dq and the same array per row for ddq, as in the reference."""
    q = to_device(q)[0].dense()
    N = q.rows
    if q.cols != model.nq:
        raise ValueError("q must have nq = %d columns, got %d" % (model.nq, q.cols))
    if N < 3:
        raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements "
                         "are required.")
    ts, dt_ptr, keep = (float(param["ts"]), None, None) if dt is None else _divisor_to_device(dt, N - 1, "dt")
    handle = _lib.ModelHandle(model.to_flat())
    dq, ddq = GpuMatrix.empty(N - 1, model.nv), GpuMatrix.empty(N - 1, model.nv)
    _lib.joint_difference(handle, N, q.ptr, ts, dt_ptr, dq.ptr)
    _lib.gradient_cols(dq.ptr, N - 1, model.nv, model.nv, min(model.nq - 1, model.nv), ts, dt_ptr, ddq.ptr, model.nv)
    del keep
    return GpuMatrix(q.buf, N - 2, model.nq), GpuMatrix(dq.buf, N - 2, model.nv), GpuMatrix(ddq.buf, N - 2, model.nv)


def median_filter_columns(data, kernel_size):
    """``signal.medfilt(data[:, c], kernel_size)`` of every column -- the first statement of the TIAGo script's
    ``apply_filters`` (examples/tiago/identification.py:63-90) -- on the device (figh_medfilt_cols).  A host array comes
    back as a host array of the same shape, a ``GpuMatrix`` as a ``GpuMatrix``."""
    kernel_size = int(kernel_size)
    if kernel_size % 2 != 1:
        raise ValueError("Each element of kernel_size should be odd.")
    on_device = isinstance(data, GpuMatrix)
    if on_device:
        X = data
    else:
        data = np.asarray(data, dtype=np.float64)
        X = GpuMatrix.from_host(data.reshape(data.shape[0], -1))
    out = GpuMatrix.empty(X.rows, X.cols)
    _lib.medfilt_cols(X.ptr, X.rows, X.cols, X.ld, 1, kernel_size, out.ptr, out.cols)
    return out if on_device else out.numpy().reshape(data.shape)


def gradient_columns(x, h):
    """``np.gradient(x[:, c], edge_order=1) / h`` of every column, ``h`` a number or one value per row (figh_gradient_cols).
    With ``h = np.gradient(t)`` this is the TIAGo script's ``estimate_acceleration``
    (examples/tiago/identification.py:92-99).  Host array in, host array out; ``GpuMatrix`` in, ``GpuMatrix`` out."""
    on_device = isinstance(x, GpuMatrix)
    if on_device:
        X = x
    else:
        x = np.asarray(x, dtype=np.float64)
        X = GpuMatrix.from_host(x.reshape(x.shape[0], -1))
    hs, h_ptr, keep = _divisor_to_device(h, X.rows, "h")
    out = GpuMatrix.empty(X.rows, X.cols)
    _lib.gradient_cols(X.ptr, X.rows, X.cols, X.ld, X.cols, hs, h_ptr, out.ptr, out.cols)
    del keep
    return out if on_device else out.numpy().reshape(x.shape)


def _filtfilt_device(x2d, nblocks, form, b, a, zi, padlen, q):
    """Columns of x2d (rows x cols, made of nblocks row blocks) through figh_filtfilt_cols; returns (rows_out, cols)."""
    x2d = np.ascontiguousarray(x2d, dtype=np.float64)
    rows, cols = x2d.shape
    d_x = _lib.DeviceArray.from_host(x2d.reshape(-1))
    L = rows // nblocks
    rows_out = ((L + q - 1) // q) * nblocks
    d_y = _lib.DeviceArray((rows_out * cols,), np.float64)
    got = _lib.filtfilt_cols(d_x, rows, cols, cols, nblocks, form, b, a, zi, padlen, q, d_y, cols)
    assert got == rows_out
    return d_y.to_host().reshape(rows_out, cols)


def low_pass_filter_data(data, param, nbutter=5):
    """Zero-phase Butterworth low-pass + border trimming -- identification_tools.py:390-424.  The filter is designed
    on the host (``signal.butter`` / ``lfilter_zi``: a dozen numbers); the forward-backward recursion over every column
    runs on the device, operation by operation as ``signal.filtfilt(b, a, data, padtype='odd', padlen=...)``.  A
    ``GpuMatrix`` comes back as a ``GpuMatrix`` (no copy to the host)."""
    from scipy import signal

    cutoff = param["ts"] * param["cut_off_frequency_butterworth"] / 2
    b, a = signal.butter(nbutter, cutoff, "low")
    padlen = 3 * (max(len(b), len(a)) - 1)
    if isinstance(data, GpuMatrix):  # stays in HBM: the trimmed result is a window of the filtered buffer
        if data.rows <= padlen:
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
        b, a = b / a[0], a / a[0]
        d_y = _lib.DeviceArray((data.rows * data.cols,), np.float64)
        _lib.filtfilt_cols(data.buf, data.rows, data.cols, data.ld, 1, 1, b, a, signal.lfilter_zi(b, a), padlen, 1, d_y,
                           data.cols)
        nbord = 5 * nbutter
        kept = max(data.rows - 2 * nbord, 0)  # (nothing left: an empty window at the start of the buffer, not past its end)
        return GpuMatrix(_DevView(d_y, 8 * nbord * data.cols if kept else 0), kept, data.cols)
    data = np.asarray(data, dtype=np.float64)
    x2d = data.reshape(data.shape[0], -1)
    if x2d.shape[0] <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    b, a = b / a[0], a / a[0]
    out = _filtfilt_device(x2d, 1, 1, b, a, signal.lfilter_zi(b, a), padlen, 1).reshape(data.shape)
    nbord = 5 * nbutter
    return out[nbord:out.shape[0] - nbord]


# ----------------------------------------------------------------------------------------------------------
# Free-flyer real data (examples/human/identification.py): the orientation filter (:330-374) and the wrench transport
# (:434-453, :471-555) on the device (csrc/figh_freeflyer.hip).  Each device function has its NumPy mirror beside it: the
# statements of the kernel element by element, in the kernel's operation order, with no BLAS product -- the function's
# definition on the host, as ``joint_difference`` is for figh_joint_difference.  Quaternions are (x y z w), 6-vectors
# (linear, angular).
_SERIES_BELOW = 2.0 ** -13           # both series of csrc/figh_freeflyer.hip
_KEEP_ABOVE = 0.7071067811865476     # cos(pi / 4): the reference's 2 acos(d) < pi / 2


def _rows_2d(x, width, what):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1 and x.shape[0] == width:
        x = x[None, :]
    if x.ndim != 2 or x.shape[1] != width or x.shape[0] < 1:
        raise ValueError("%s: expected (N, %d) with N >= 1, got shape %r" % (what, width, x.shape))
    return x


def quaternion_log_mirror(quat):
    """figh_quat_log on the host: n = sqrt((x x + y y) + z z), r = sgn(w) (2 atan2(n, |w|) / n) (x, y, z) with sgn(0) = +1,
    the series 2 ((1 - t^2 / 3) + t^4 / 5) / |w|, t = n / |w|, for n < 2^-13 |w|, three +0.0 for n = 0."""
    quat = _rows_2d(quat, 4, "quaternion_log")
    x, y, z, w = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    n, aw = np.sqrt((x * x + y * y) + z * z), np.abs(w)
    s = np.where(w < 0.0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        t = n / aw
        t2 = t * t
        series = 2.0 * ((1.0 - t2 / 3.0) + (t2 * t2) / 5.0) / aw
        f = np.where(n < _SERIES_BELOW * aw, series, 2.0 * np.arctan2(n, aw) / n)
        sf = s * f
        out = np.stack([sf * x, sf * y, sf * z], axis=1)
    out[n == 0.0] = 0.0
    return out


def rotation_vector_to_quaternion_mirror(rotvec, quat_ref):
    """figh_rotvec_to_quat on the host: the canonical quaternion of exp3(r), Eigen's representative of it, and the
    reference's sign test against ``quat_ref`` (keep iff d > 0.7071067811865476; d > 1 by rounding keeps)."""
    rotvec, ref = _rows_2d(rotvec, 3, "rotation_vector_to_quaternion"), _rows_2d(quat_ref, 4, "rotation_vector_to_quaternion")
    if len(rotvec) != len(ref):
        raise ValueError("rotation_vector_to_quaternion: %d rotation vectors, %d reference quaternions" % (len(rotvec), len(ref)))
    rx, ry, rz = rotvec[:, 0], rotvec[:, 1], rotvec[:, 2]
    th2 = (rx * rx + ry * ry) + rz * rz
    th = np.sqrt(th2)
    th4 = th2 * th2
    with np.errstate(all="ignore"):
        small = th < _SERIES_BELOW
        a = np.where(small, (0.5 - th2 / 48.0) + th4 / 3840.0, np.sin(0.5 * th) / th)
        c = np.where(small, (1.0 - th2 / 8.0) + th4 / 384.0, np.cos(0.5 * th))
    q0, q1, q2 = a * rx, a * ry, a * rz
    lead = q0.copy()
    lead = np.where(np.abs(q1) > np.abs(lead), q1, lead)
    lead = np.where(np.abs(q2) > np.abs(lead), q2, lead)
    lead = np.where(np.abs(c) > 0.5, c, lead)
    sE = np.where(lead < 0.0, -1.0, 1.0)
    d = sE * (((q0 * ref[:, 0] + q1 * ref[:, 1]) + q2 * ref[:, 2]) + c * ref[:, 3])
    sg = np.where(d > _KEEP_ABOVE, sE, -sE)
    return np.stack([sg * q0, sg * q1, sg * q2, sg * c], axis=1)


def _rot_rows(R, x, transpose=False):
    """y = R x (R^T x), R (..., 3, 3), x a list of three arrays: three products summed left to right, like figh_spatial.h."""
    if transpose:
        return [R[..., 0, r] * x[0] + R[..., 1, r] * x[1] + R[..., 2, r] * x[2] for r in range(3)]
    return [R[..., r, 0] * x[0] + R[..., r, 1] * x[1] + R[..., r, 2] * x[2] for r in range(3)]


def _matmul3_rows(A, B):
    """A B entry by entry, A (..., 3, 3) or (3, 3), B (N, 3, 3): matmul3 of figh_spatial.h."""
    C = np.empty(B.shape)
    for r in range(3):
        for c in range(3):
            C[:, r, c] = A[..., r, 0] * B[:, 0, c] + A[..., r, 1] * B[:, 1, c] + A[..., r, 2] * B[:, 2, c]
    return C


def _cross_rows(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _joint_id(model, joint):
    j = model.getJointId(joint) if isinstance(joint, str) else int(joint)
    if not 0 <= j < model.njoints:
        raise ValueError("transport_wrench: joint %r is not in the model" % (joint,))
    return j


def joint_world_placement_mirror(model, q, joint):
    """(R, p) = oMi[joint](q_i), (N, 3, 3) and (N, 3), as figh_wrench_transport composes it: root first,
    (Rk, pk) = placement_j . M_j(q_j), (R, p) = (Rk, pk) at the first joint, then (R Rk, p + R pk)."""
    from ..calibration.calibration_tools import _joint_motion

    q = np.asarray(q, dtype=np.float64)
    N = q.shape[0]
    path, j = [], _joint_id(model, joint)
    while j > 0:
        path.append(j)
        j = model.parents[j]
    R = np.broadcast_to(np.eye(3), (N, 3, 3)).copy()
    p = np.zeros((N, 3))
    for s, j in enumerate(path[::-1]):
        Rj, pj = _joint_motion(model.joints[j], q)
        pl = model.jointPlacements[j]
        Pr, Pt = np.asarray(pl.rotation, dtype=np.float64), np.asarray(pl.translation, dtype=np.float64)
        Rk = _matmul3_rows(Pr, Rj)
        pk = np.stack(_rot_rows(Pr, [pj[:, 0], pj[:, 1], pj[:, 2]]), axis=1) + Pt[None, :]
        if s == 0:
            R, p = Rk, pk
        else:
            t = _rot_rows(R, [pk[:, 0], pk[:, 1], pk[:, 2]])
            R = _matmul3_rows(R, Rk)
            p = p + np.stack(t, axis=1)
    return R, p


_WRENCH_LAYOUTS = ("sample", "stacked")


def _check_layouts(layout_in, layout_out):
    for name in (layout_in, layout_out):
        if name not in _WRENCH_LAYOUTS:
            raise ValueError("transport_wrench: unknown layout %r (one of %r)" % (name, _WRENCH_LAYOUTS))


def _wrench_components(wrench, N, layout):
    """The six component arrays (N,) of a host wrench array in ``layout``."""
    w = np.asarray(wrench, dtype=np.float64)
    if layout == "sample":
        if w.shape != (N, 6):
            raise ValueError("transport_wrench: the sample layout is (N, 6) = (%d, 6), got shape %r" % (N, w.shape))
        return [w[:, k] for k in range(6)]
    if w.reshape(-1).shape[0] != 6 * N or w.ndim != 1:
        raise ValueError("transport_wrench: the stacked layout has 6 N = %d entries, got shape %r" % (6 * N, w.shape))
    return [w[k * N:(k + 1) * N] for k in range(6)]


def _as_samples(model, q):
    q = np.asarray(q, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != model.nq or q.shape[0] < 1:
        raise ValueError("expected q of shape (N, nq = %d) with N >= 1, got %r" % (model.nq, q.shape))
    return q


def transport_wrench_mirror(model, q, wrench, joint="root_joint", inverse=False, layout_in="sample", layout_out="stacked"):
    """figh_wrench_transport on the host.  ``inverse=False``: pin.Force.se3Action(oMi[joint]), f' = R f,
    n' = R n + p x f'; ``inverse=True``: se3ActionInverse, f' = R^T f, n' = R^T (n - p x f)."""
    _check_layouts(layout_in, layout_out)
    q = _as_samples(model, q)
    N = q.shape[0]
    w = _wrench_components(wrench, N, layout_in)
    R, p = joint_world_placement_mirror(model, q, _joint_id(model, joint))
    f, n, pp = w[:3], w[3:], [p[:, 0], p[:, 1], p[:, 2]]
    if inverse:
        c = _cross_rows(pp, f)
        m = [n[d] - c[d] for d in range(3)]
        o = _rot_rows(R, f, transpose=True) + _rot_rows(R, m, transpose=True)
    else:
        fo = _rot_rows(R, f)
        m = _rot_rows(R, n)
        c = _cross_rows(pp, fo)
        o = fo + [m[d] + c[d] for d in range(3)]
    return np.stack(o, axis=1) if layout_out == "sample" else np.concatenate(o)


def _device_rows(x, width, what):
    """(GpuMatrix, was_resident) of an (N, width) host array or GpuMatrix."""
    if isinstance(x, GpuMatrix):
        if x.cols != width or x.rows < 1:
            raise ValueError("%s: expected (N, %d) with N >= 1, got %r" % (what, width, x.shape))
        return x, True
    return GpuMatrix.from_host(_rows_2d(x, width, what)), False


def quaternion_log(quat):
    """``pin.log3(pin.Quaternion(quat[i]))`` of every row (examples/human/identification.py:330-339) on the device
    (figh_quat_log): the principal rotation vector, (N, 3).  ``quat``: (N, 4) quaternions (x y z w), a host array (a host
    array comes back) or a ``GpuMatrix`` of four columns with any leading dimension -- a window of q is
    ``GpuMatrix(_DevView(q.buf, 8 * (idx_q + 3)), N, 4, q.ld)`` -- which gives a resident ``GpuMatrix``.  q and -q give the
    same vector; where w changes sign at theta = pi the vector jumps as the reference's does (nothing unwraps it).
    Host definition: :func:`quaternion_log_mirror`."""
    Q, resident = _device_rows(quat, 4, "quaternion_log")
    out = GpuMatrix.empty(Q.rows, 3)
    _lib.quat_log(Q.ptr, Q.rows, Q.ld, out.ptr, 3)
    return out if resident else out.numpy()


def rotation_vector_to_quaternion(rotvec, quat_ref):
    """``pin.Quaternion(pin.exp3(rotvec[i]))`` with the sign the script chooses against ``quat_ref[i]``
    (examples/human/identification.py:349-364) on the device (figh_rotvec_to_quat), (N, 4).  The representative is Eigen's
    (w > 0 when |w| > 1/2, else the largest vector component positive), kept when its dot product d with the reference
    exceeds cos(pi / 4) and negated otherwise.  The one deliberate difference from the script: when rounding makes d > 1
    its ``arccos`` is NaN and it negates; here that case keeps -- rounding noise decides it, and -q is the same rotation.
    Host arrays in, host array out; a ``GpuMatrix`` rotvec gives a resident ``GpuMatrix``.
    Host definition: :func:`rotation_vector_to_quaternion_mirror`."""
    what = "rotation_vector_to_quaternion"
    rotvec, quat_ref = (x if isinstance(x, GpuMatrix) else _rows_2d(x, w, what) for x, w in ((rotvec, 3), (quat_ref, 4)))
    if len(rotvec) != len(quat_ref):
        raise ValueError("%s: %d rotation vectors, %d reference quaternions" % (what, len(rotvec), len(quat_ref)))
    Rv, resident = _device_rows(rotvec, 3, what)
    Qr, _ = _device_rows(quat_ref, 4, what)
    out = GpuMatrix.empty(Rv.rows, 4)
    _lib.rotvec_to_quat(Rv.ptr, Rv.rows, Rv.ld, Qr.ptr, Qr.ld, out.ptr, 4)
    return out if resident else out.numpy()


def _free_flyers(model):
    return [j for j in model.joints[1:] if j.jtype == 3]


def filter_free_flyer_mirror(model, q, param, nbutter=5):
    """:func:`filter_free_flyer` on the host: ``scipy.signal.filtfilt`` (what the reference's low_pass_filter_data calls) and
    the mirrors of the logarithm and the exponential, with the same row pairing."""
    from scipy import signal

    q = _as_samples(model, q)
    b, a = signal.butter(nbutter, param["ts"] * param["cut_off_frequency_butterworth"] / 2, "low")
    padlen, nbord = 3 * (max(len(b), len(a)) - 1), 5 * nbutter

    def low_pass(x):
        y = signal.filtfilt(b, a, x, axis=0, padtype="odd", padlen=padlen)
        return y[nbord:y.shape[0] - nbord]

    q_f = np.ascontiguousarray(low_pass(q))
    for j in _free_flyers(model):
        lo = j.idx_q + 3
        rotvec = low_pass(quaternion_log_mirror(q[:, lo:lo + 4]))
        if len(rotvec):
            q_f[:, lo:lo + 4] = rotation_vector_to_quaternion_mirror(rotvec, q[:len(rotvec), lo:lo + 4])
    return q_f


def filter_free_flyer(model, q, param, nbutter=5):
    """The free-flyer orientation filter of examples/human/identification.py:330-374, resident from q to q: every column of
    ``q`` goes through :func:`low_pass_filter_data`; for every free-flyer joint the rotation vector of its quaternion
    (:func:`quaternion_log`) goes through it too, is turned back into a quaternion
    (:func:`rotation_vector_to_quaternion`) and written over the filtered quaternion columns in place (``q_m[:, 3:7] =
    quat_filt``).  Returns the filtered configurations, ``len(q) - 10 nbutter`` rows.

    ROW PAIRING: the script's own.  ``low_pass_filter_data`` trims 5 nbutter rows at each border, so row ``ii`` of the
    filtered signal is sample ``ii + 5 nbutter`` -- and the script chooses its sign against ``q_mocap[ii]``, the RAW row
    ``ii``, not ``ii + 5 nbutter``.  A drop-in keeps that.

    A host array comes back as a host array; a ``GpuMatrix`` (any leading dimension) stays in HBM and a ``GpuMatrix`` comes
    back, ready for :func:`calculate_first_second_order_differentiation`.  Host definition:
    :func:`filter_free_flyer_mirror`."""
    resident = isinstance(q, GpuMatrix)
    Q = q if resident else GpuMatrix.from_host(_as_samples(model, q))
    if Q.cols != model.nq or Q.rows < 1:
        raise ValueError("expected q of shape (N, nq = %d) with N >= 1, got %r" % (model.nq, Q.shape))
    q_f = low_pass_filter_data(Q, param, nbutter)
    for j in _free_flyers(model):
        off = 8 * (j.idx_q + 3)
        rotvec = GpuMatrix.empty(Q.rows, 3)
        _lib.quat_log(Q.ptr + off, Q.rows, Q.ld, rotvec.ptr, 3)
        rotvec_f = low_pass_filter_data(rotvec, param, nbutter)
        if rotvec_f.rows:
            _lib.rotvec_to_quat(rotvec_f.ptr, rotvec_f.rows, rotvec_f.ld, Q.ptr + off, Q.ld, q_f.ptr + off, q_f.ld)
    return q_f if resident else q_f.numpy()


def transport_wrench(model, q, wrench, joint="root_joint", inverse=False, layout_in="sample", layout_out="stacked"):
    """A wrench per sample carried through ``oMi[joint](q_i)`` on the device (figh_wrench_transport).
    ``inverse=True`` is ``pin.Force.se3ActionInverse`` -- the measured force-plate wrench from the world frame into the
    pelvis frame, examples/human/identification.py:434-453 --, ``inverse=False`` is ``se3Action`` -- the simulated and
    identified wrenches back to the world frame, :471-555.  ``joint``: a joint name or id, any joint of the model.

    Layouts: "sample" is (N, 6), (linear, angular) per row; "stacked" is the vector ``[k N + i]``, the order of ``tau`` and of
    ``regressor_times_parameters``.  Host arrays in, host array out.  A ``GpuMatrix`` q, a ``GpuMatrix`` wrench (sample layout) or
    a device vector (stacked layout) gives a resident result with no download: a ``GpuMatrix`` (sample) or a ``DeviceArray``
    (stacked), which ``IdentificationPipeline.set_samples(tau=...)`` takes as it is.
    Host definition: :func:`transport_wrench_mirror`."""
    _check_layouts(layout_in, layout_out)
    j = _joint_id(model, joint)
    wrench_resident = isinstance(wrench, GpuMatrix) or hasattr(wrench, "ptr")
    resident = isinstance(q, GpuMatrix) or wrench_resident
    if not isinstance(q, GpuMatrix):
        q = _as_samples(model, q)
    elif q.cols != model.nq or q.rows < 1:
        raise ValueError("expected q of shape (N, nq = %d) with N >= 1, got %r" % (model.nq, q.shape))
    N = len(q)
    if wrench_resident:
        if layout_in == "sample":
            if not isinstance(wrench, GpuMatrix) or wrench.shape != (N, 6) or wrench.ld != 6:
                raise ValueError("transport_wrench: a resident wrench in the sample layout is a dense GpuMatrix (%d, 6)" % N)
        elif isinstance(wrench, GpuMatrix) or int(getattr(wrench, "size", 6 * N)) != 6 * N:
            raise ValueError("transport_wrench: a resident wrench in the stacked layout is a device vector of 6 N = %d entries"
                             % (6 * N))
        d_F = wrench
    else:
        _wrench_components(wrench, N, layout_in)  # (the shape check)
        d_F = _lib.DeviceArray.from_host(np.ascontiguousarray(wrench, dtype=np.float64).reshape(-1))
    Q = q if isinstance(q, GpuMatrix) else GpuMatrix.from_host(q)
    handle = _lib.ModelHandle(model.to_flat())
    out = GpuMatrix.empty(N, 6) if layout_out == "sample" else _lib.DeviceArray((6 * N,), np.float64)
    _lib.wrench_transport(handle, j, N, Q.ptr, Q.ld, d_F.ptr, layout_in, inverse, out.ptr, layout_out)
    if resident:
        return out
    return out.numpy() if layout_out == "sample" else out.to_host()


def _decimate_design(q, n=8):
    """The IIR of ``scipy.signal.decimate(ftype='iir')``: Chebyshev-I order 8, 0.05 dB, 0.8/q, as second-order
    sections, with SciPy's padlen rule for sosfiltfilt."""
    from scipy import signal

    sos = signal.cheby1(n, 0.05, 0.8 / q, output="sos")
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())
    return sos, signal.sosfilt_zi(sos), 3 * ntaps


class _DevView:
    """A window into a device buffer (no ownership; keeps its base alive)."""

    def __init__(self, base, byte_offset):
        self.base = base
        self.ptr = base.ptr + int(byte_offset)


def _decimate_device(W, tau, nblocks, q, stages, blocks=None):
    """decimate_joint_blocks for a regressor that lives in HBM: the stages run device buffer to device buffer
    (figh_filtfilt_cols), the blocks come back as GpuMatrix / device-vector views of one stacked result."""
    sos, zi, padlen = _decimate_design(q)
    d_tau = vector_to_device(tau)
    ntau = getattr(d_tau, "size", None) or len(tau)
    nj = ntau // nblocks
    if blocks is not None:
        # active joints: tau block i goes with the rows [blocks[i] nj, (blocks[i] + 1) nj) of W -- gathered into one stack on
        # the device (a copy of the active blocks only), then decimated like a regressor that has just these blocks
        if W.rows < (max(blocks) + 1) * nj:
            raise ValueError("device-resident decimation needs W to cover row block %d" % max(blocks))
        stack = GpuMatrix.empty(nblocks * nj, W.cols)
        lib = _lib.load()
        for i, b in enumerate(blocks):
            if W.ld == W.cols:
                _lib.check(lib.figh_memcpy_d2d(stack.buf.ptr + 8 * i * nj * W.cols, W.buf.ptr + 8 * b * nj * W.ld,
                                               8 * nj * W.cols))
            else:
                _lib.place_block(W.buf.ptr + 8 * b * nj * W.ld, W.ld, nj, W.cols, 1.0,
                                 stack.buf.ptr + 8 * i * nj * W.cols, W.cols)
        W = stack
    if W.rows < nblocks * nj:
        raise ValueError("device-resident decimation needs W to cover the %d joint blocks of tau" % nblocks)

    def run(buf, rows, cols, ld):
        for _ in range(stages):
            L = rows // nblocks
            if L <= padlen:
                raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
            rows_out = ((L + q - 1) // q) * nblocks
            d_y = _lib.DeviceArray((rows_out * cols,), np.float64)
            got = _lib.filtfilt_cols(buf, rows, cols, ld, nblocks, 0, sos[:, :3], sos[:, 3:], zi, padlen, q, d_y, cols)
            assert got == rows_out
            buf, rows, ld = d_y, rows_out, cols
        return buf, rows

    t_buf, t_rows = run(d_tau, nblocks * nj, 1, 1)
    w_buf, w_rows = run(W.buf, nblocks * nj, W.cols, W.ld)
    lt, lw = t_rows // nblocks, w_rows // nblocks
    W_list = [GpuMatrix(_DevView(w_buf, 8 * i * lw * W.cols), lw, W.cols) for i in range(nblocks)]
    tau_list = [_DevView(t_buf, 8 * i * lt) for i in range(nblocks)]
    for t in tau_list:
        t.size = lt
    return W_list, tau_list


def reject_rows(W_list, tau_list, key_cols, thresholds):
    """Zero-velocity row rejection of the real-data scripts (examples/staubli_TX40/identification.py:207-233,
    examples/tiago/identification.py:170-187): from joint block i the rows with ``|W_i[:, key_cols[i]]| < thresholds[i]``
    are dropped (W and tau alike), the surviving blocks are stacked.  Returns (W_, tau_, counts).

    GpuMatrix blocks (decimate_joint_blocks on a device-resident W) are compacted on the device
    (figh_compact_rows: order-preserving stream compaction) into one GpuMatrix / device vector -- nothing but the six
    counts returns to the host; NumPy blocks are filtered with NumPy, as in the scripts."""
    nb = len(W_list)
    if not (len(tau_list) == len(key_cols) == len(thresholds) == nb):
        raise ValueError("one key column and one threshold per joint block")
    if not isinstance(W_list[0], GpuMatrix):
        Wk, tk, counts = [], [], []
        for i in range(nb):
            keep = np.abs(np.asarray(W_list[i])[:, key_cols[i]]) >= thresholds[i]
            Wk.append(np.asarray(W_list[i])[keep])
            tk.append(np.asarray(tau_list[i])[keep])
            counts.append(int(keep.sum()))
        return np.vstack(Wk), np.concatenate(tk), counts
    cols = W_list[0].cols
    total = sum(w.rows for w in W_list)
    out = GpuMatrix.empty(total, cols)
    d_tau = _lib.DeviceArray((max(total, 1),), np.float64)
    counts, at = [], 0
    for i in range(nb):
        w = W_list[i]
        kept = _lib.compact_rows(w.ptr, w.rows, cols, w.ld, tau_list[i].ptr, int(key_cols[i]), float(thresholds[i]),
                                 out.ptr + 8 * at * cols, cols, d_tau.ptr + 8 * at)
        counts.append(int(kept))
        at += int(kept)
    out.rows = at
    d_tau.size, d_tau.shape = at, (at,)
    d_tau.nbytes = 8 * at
    return out, d_tau, counts


def essential_parameters(R_ols, R_wls, params_base, std_xr, ratio_essential, rows_total=None):
    """The essential-parameter loop of examples/staubli_TX40/identification.py:354-399 on the two small triangles a pass
    leaves behind instead of on W: ``R_ols`` = the (r + 1) x (r + 1) R factor of [W_b tau], ``R_wls`` = that of
    [S^-1/2 W_b, S^-1/2 tau] with the per-joint variances of the full-base WLS (the script keeps using THOSE variances
    inside the loop: ``diag_SIGMA_e`` is filled from ``sig_ro_joint``, not from ``sig_ro_joint_e``).  Deleting a column of W_b
    deletes the same column of both triangles, and every quantity of an iteration -- lstsq, relative_stdev, C_X, the WLS
    solution -- follows from the re-triangularised r x r remainder: the rows of W are never read again.

    While ``max(std) >= ratio_essential * min(std)``: drop the parameter with the largest std% (``np.isclose`` match, as in
    the script; a TIE -- two parameters whose 2-decimal std% are both "the largest", two ``inf`` included -- raises
    TypeError exactly where the script's ``int(i)`` does, instead of silently dropping the first), OLS (6 decimals) + its std%,
    WLS (6 decimals) + its std%.  ``rows_total`` = len(tau_) (the row count relative_stdev divides by; without it
    std_e_ols is left out).  Returns a dict: params_essential, idx_essential (positions in params_base), phi_e_ols,
    std_e_ols, phi_e_wls, std_e_wls, iterations."""
    R_ols = np.triu(np.asarray(R_ols, dtype=np.float64))
    R_wls = np.triu(np.asarray(R_wls, dtype=np.float64))
    r = R_ols.shape[0] - 1
    if R_wls.shape != R_ols.shape or len(params_base) != r or len(std_xr) != r:
        raise ValueError("essential_parameters: triangles, names and std% must describe the same %d parameters" % r)
    keep = list(range(r))
    names = list(params_base)
    std_e = np.asarray(std_xr, dtype=np.float64).copy()
    out = {"phi_e_ols": None, "std_e_ols": None, "phi_e_wls": None, "std_e_wls": None}
    it = 0
    while not (std_e.max() < ratio_essential * std_e.min()):
        (i,) = np.where(np.isclose(std_e, std_e.max()))
        if i.size != 1:  # the script: int(i) of a longer array
            raise TypeError("only length-1 arrays can be converted to Python scalars (essential_parameters: %d parameters "
                            "tie for the largest std%% %r)" % (i.size, float(std_e.max())))
        del names[int(i[0])]
        del keep[int(i[0])]
        k = len(keep)

        def sub(R):  # R factor of the remaining columns [+ tau]
            return np.linalg.qr(R[:, keep + [r]], mode="r")
        Ro, Rw = sub(R_ols), sub(R_wls)
        phi_o = np.around(np.linalg.solve(Ro[:k, :k], Ro[:k, k]), 6)
        out["phi_e_ols"] = phi_o
        if rows_total is not None:  # relative_stdev (identification_tools.py:204-234) of (W_essential, phi_e_ols, tau_)
            res2 = float(np.sum((Ro[:k, :k] @ phi_o - Ro[:k, k]) ** 2) + (Ro[k, k] ** 2 if Ro.shape[0] > k else 0.0))
            Ri = np.linalg.inv(Ro[:k, :k])
            C = res2 / (rows_total - k) * (Ri @ Ri.T)
            out["std_e_ols"] = relative_percent(np.sqrt(np.diag(C)), phi_o)
        Rwi = np.linalg.inv(Rw[:k, :k])
        phi_w = np.around(np.linalg.solve(Rw[:k, :k], Rw[:k, k]), 6)
        std_e = relative_percent(np.sqrt(np.einsum("ij,ij->i", Rwi, Rwi)), phi_w)
        out["phi_e_wls"], out["std_e_wls"] = phi_w, std_e.copy()
        it += 1
    out.update(params_essential=names, idx_essential=keep, iterations=it)
    return out



def decimate_joint_blocks(W, tau, nblocks, q=10, stages=2, blocks=None):
    """Per-joint decimation of tau and of every column of W with ``scipy.signal.decimate(zero_phase=True)``
    (examples/staubli_TX40/identification.py:186-204, examples/tiago/identification.py:142-187).
    Returns (list of W blocks, list of tau blocks).  Block i of W is ``W[i*nj:(i+1)*nj]`` with nj taken from tau, as in
    the scripts (when tau is longer than W's joint blocks the W blocks are offset and the last one is shorter -- kept).
    Every (block, column) sequence is one device thread running SciPy's sosfiltfilt recurrences;
    equal-length blocks share a launch.

    A ``GpuMatrix`` W (``param["device_resident"]``) stays in HBM: the blocks come back as GpuMatrix views and device
    vectors (for :func:`reject_rows`), nothing is copied to the host.

    ``blocks`` (ACTIVE JOINTS, examples/tiago/identification.py:148-187: ``act_idxv``): W is the regressor of ALL dofs, tau
    holds the ``nblocks = len(blocks)`` measured joints only, and block i of the result is the decimated row block
    ``blocks[i]`` of W -- ``W[blocks[i]*nj:(blocks[i]+1)*nj]`` -- the other row blocks are never touched.  The TIAGo script
    decimates once (``stages=1``)."""
    if blocks is not None:
        blocks = [int(b) for b in blocks]
        if len(blocks) != nblocks:
            raise ValueError("decimate_joint_blocks: %d blocks listed, nblocks = %d" % (len(blocks), nblocks))
    if isinstance(W, GpuMatrix):
        return _decimate_device(W, tau, nblocks, q, stages, blocks)
    W = np.asarray(W, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    nj = tau.shape[0] // nblocks
    if blocks is not None:
        if W.shape[0] < (max(blocks) + 1) * nj:
            raise ValueError("decimate_joint_blocks: W does not cover row block %d" % max(blocks))
        W = np.concatenate([W[b * nj:(b + 1) * nj] for b in blocks])  # the active blocks only, in the listed order
    sos, zi, padlen = _decimate_design(q)

    def run(x2d, nb):  # nb equal blocks stacked in x2d
        for _ in range(stages):
            if x2d.shape[0] // nb <= padlen:
                raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
            x2d = _filtfilt_device(x2d, nb, 0, sos[:, :3], sos[:, 3:], zi, padlen, q)
        return x2d

    t = run(tau[:nj * nblocks].reshape(-1, 1), nblocks)
    lt = t.shape[0] // nblocks
    tau_list = [np.ascontiguousarray(t[i * lt:(i + 1) * lt, 0]) for i in range(nblocks)]
    lengths = [max(0, min(W.shape[0], (i + 1) * nj) - i * nj) for i in range(nblocks)]
    W_list = [None] * nblocks
    i = 0
    while i < nblocks:  # consecutive blocks of equal length go through one launch
        k = i
        while k + 1 < nblocks and lengths[k + 1] == lengths[i]:
            k += 1
        nb = k - i + 1
        y = run(W[i * nj:i * nj + nb * lengths[i]], nb)
        ly = y.shape[0] // nb
        for b in range(nb):
            W_list[i + b] = np.ascontiguousarray(y[b * ly:(b + 1) * ly])
        i = k + 1
    return W_list, tau_list


@host_tail
def sip_qp_terms(robot, q, v, a, tau, param, col_idx, phi_ref, alpha, coupling=False, exchange=None):
    """The data terms of ``calculate_standard_parameters`` (identification_tools.py:466-572, the SIP quadratic
    program): ``P = (1-alpha) sf1 I + alpha sf2 W^T W`` and ``r = -((1-alpha) sf1 phi_ref + alpha sf2 W^T tau)`` with
    ``sf1 = 1 / (max(phi_ref) len(phi_ref))``, ``sf2 = 1 / (max(tau) len(tau))`` (``:528-531``), for the columns
    ``col_idx`` of the regressor of the samples (q, v, a).  W^T W and W^T tau come from ``figh_regressor_gram`` (formed
    from the Householder triangle, W never stored); the constraint matrices G, h and the QP solve (quadprog) stay with
    the caller.  Returns (P, r).

    ``exchange`` (figaroh_plus_amd.dist, one process per GPU): (q, v, a, tau) are THIS rank's shard of the samples; the
    Gram terms of all shards are summed in one all-reduce (``dist.allreduce_normal_terms``: collective (1) of SURVEY 8e),
    ``max(tau)`` and ``len(tau)`` are taken over all ranks, and every rank returns the same (P, r) as a single process
    would on the whole sample set."""
    from ..tools.regressor import _samples_to_device, regressor_flags

    mode, flags, ft_mask = regressor_flags(param, coupling)
    dm = robot.device_model()
    cols = np.ascontiguousarray(col_idx, dtype=np.int32)
    n = len(cols)
    phi_ref = np.asarray(phi_ref, dtype=np.float64)
    tau = np.ascontiguousarray(tau, dtype=np.float64)
    if phi_ref.shape != (n,):
        raise ValueError("phi_ref must have one entry per selected column")
    N, d_q, d_v, d_a = _samples_to_device(robot.model, q, v, a)
    d_idx = _lib.DeviceArray.from_host(cols)
    d_tau = _lib.DeviceArray.from_host(tau)
    G, g, tt = _lib.regressor_gram(dm, mode, flags, ft_mask, N, d_q, d_v, d_a, d_idx, n, d_tau)
    tau_max, tau_len = np.max(tau), len(tau)
    if exchange is not None and exchange.world_size > 1:
        from ..dist import allgather_max, allreduce_normal_terms
        _, G, g, tt, tau_len = allreduce_normal_terms(exchange, None, G, g, tt, tau_len)
        tau_max = allgather_max(exchange, tau_max)
    sf1 = 1 / (np.max(phi_ref) * len(phi_ref))
    sf2 = 1 / (tau_max * tau_len)
    P = (1 - alpha) * sf1 * np.eye(n) + alpha * sf2 * G
    r = -((1 - alpha) * sf1 * phi_ref + sf2 * alpha * g)
    return P, r


def quadprog_solve_qp(P, q, G=None, h=None, A=None, b=None):
    """``minimize 1/2 x^T P x + q^T x  s.t.  G x <= h, A x = b`` -- identification_tools.py:429-463, statement by
    statement; the Goldfarb-Idnani solve itself is ``qp.solve_qp`` (quadprog is a third-party dependency of the
    reference)."""
    from .qp import solve_qp

    n = P.shape[0]
    qp_G = 0.5 * (P + P.T) + 1e-5 * np.eye(n)  # symmetrised and shifted: strictly convex whatever the data
    eq = A is not None
    rows = np.vstack([A, G]) if eq else G
    rhs = np.hstack([b, h]) if eq else h
    # quadprog's convention is C^T x >= b: both signs flip
    return solve_qp(qp_G, -q, -rows.T, -rhs, A.shape[0] if eq else 0)[0]


def sip_constraints(phi_ref, COM_max, COM_min):
    """G, h of identification_tools.py:533-566: 14 bound rows per massed body -- first moments inside
    [COM_min, COM_max], mass and Ixx, Iyy, Izz inside [0.7, 1.3] x their reference values."""
    phi_ref = np.asarray(phi_ref, dtype=np.float64)
    nreal = phi_ref.shape[0] // 10
    G = np.zeros((14 * nreal, 10 * nreal))
    h = np.zeros(14 * nreal)
    for ii in range(nreal):
        for k in range(3):  # mx, my, mz
            G[14 * ii + 2 * k, ii * 10 + 6 + k] = 1
            h[14 * ii + 2 * k] = COM_max[3 * ii + k]
            G[14 * ii + 2 * k + 1, ii * 10 + 6 + k] = -1
            h[14 * ii + 2 * k + 1] = -COM_min[3 * ii + k]
        for k, col in enumerate((9, 0, 3, 5)):  # m, Ixx, Iyy, Izz
            G[14 * ii + 6 + 2 * k, ii * 10 + col] = 1
            h[14 * ii + 6 + 2 * k] = 1.3 * phi_ref[ii * 10 + col]
            G[14 * ii + 7 + 2 * k, ii * 10 + col] = -1
            h[14 * ii + 7 + 2 * k] = -0.7 * phi_ref[ii * 10 + col]
    return G, h


@host_tail
def calculate_standard_parameters(model, W, tau, COM_max, COM_min, params_standard_u, alpha):
    """(phi_standard, phi_ref) -- identification_tools.py:466-572: the standard inertial parameters that fit the
    measurements (weight alpha), stay near the URDF values (weight 1 - alpha) and keep first moments, masses and
    principal inertias inside their bounds.  ``W`` (host array or ``GpuMatrix``, 10 columns per massed body) is
    reduced on the device: ``W^T W`` and ``W^T tau`` are formed from the Householder triangle of ``[W tau]``
    (``figh_tsqr``); the 10 nreal-variable program is solved on the host."""
    phi_ref = []
    id_inertias = [jj for jj in range(len(model.inertias)) if model.inertias[jj].mass != 0]
    nreal = len(id_inertias)
    params_name = ("Ixx", "Ixy", "Ixz", "Iyy", "Iyz", "Izz", "mx", "my", "mz", "m")
    for k in range(nreal):
        for j in params_name:
            phi_ref.append(params_standard_u[j + str(id_inertias[k])])
    phi_ref = np.array(phi_ref)
    tau = np.ascontiguousarray(tau, dtype=np.float64).reshape(-1)
    Wd, _ = to_device(W)
    n = Wd.cols
    if n != 10 * nreal:
        raise ValueError("W has %d columns, the model has %d bodies with mass (10 columns each)" % (n, nreal))
    R = rfactor(Wd, tau=tau)  # [R z; 0 rho]: W^T W = R^T R, W^T tau = R^T z
    WtW = R[:n, :n].T @ R[:n, :n]
    Wttau = R[:n, :n].T @ R[:n, n]
    sf1 = 1 / (np.max(phi_ref) * len(phi_ref))
    sf2 = 1 / (np.max(tau) * len(tau))
    P = (1 - alpha) * sf1 * np.eye(n) + alpha * sf2 * WtW
    r = -((1 - alpha) * sf1 * phi_ref.T + sf2 * alpha * Wttau)
    G, h = sip_constraints(phi_ref, COM_max, COM_min)
    phi_standard = quadprog_solve_qp(P, r, G, h)
    return phi_standard, phi_ref
