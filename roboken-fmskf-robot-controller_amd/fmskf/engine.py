"""Python host mirror of the C ABI: one Engine = one fmskf handle = N robots.

Inputs may be numpy arrays (host memory; copied to the device on the handle's
stream) or torch CUDA tensors (device memory, zero copy).  Outputs are numpy
arrays (host readout synchronises the stream).  Array layouts are the SoA
planes documented in include/fmskf.h.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MEM_DEVICE, MEM_HOST, MODEL_EKF9, MODEL_KF6, MODEL_KF12D, MODEL_NAMES,
                   MODEL_RS, TRIG_LIBM, TRIG_TABLE512, Config, CtrlParams, ENOTSUP, FIX_HEADING, FmskfError,
                   EKF9_ROWS, Gate, PoseFixParams, RANGE_ANCHORS_MAX, RangeParams, ROW_GATE_D2, RowGate, SEL_GATE_RUN,
                   SEL_NONFINITE, SEL_POS_VAR, SelectParams, TickInputs, check, load)

# fmskf_vehicle_info (include/fmskf.h): the VehicleInfo message layout, 84 bytes
VEHICLE_INFO_DTYPE = np.dtype([("pos_x", "<i4"), ("pos_y", "<i4"), ("pos_theta", "<f4"),
                               ("vel_x", "<i4"), ("vel_y", "<i4"), ("vel_theta", "<f4"),
                               ("imu_fault", "u1"), ("pad_", "u1", 3), ("imu_q", "<f4", 4),
                               ("imu_g", "<f4", 3), ("imu_a", "<f4", 3), ("floor", "u1", 8),
                               ("cam_pitch", "<f4"), ("fault", "<u4")])

# fmskf_kf6_record (include/fmskf.h): one robot's KF6 tick record, 16 bytes
KF6_RECORD_DTYPE = np.dtype([("yaw_deg", "<f4"), ("gyro_z_dps", "<f4"), ("rpm", "<i2", 4)])

# fmskf_pose_fix (include/fmskf.h): one absolute pose fix, 16 bytes
POSE_FIX_DTYPE = np.dtype([("robot", "<u4"), ("x_m", "<f4"), ("y_m", "<f4"), ("theta_rad", "<f4")])

# fmskf_range_fix (include/fmskf.h): one measured range to one anchor, 16 bytes
RANGE_FIX_DTYPE = np.dtype([("robot", "<u4"), ("anchor", "<u4"), ("range_m", "<f4"), ("var_m2", "<f4")])

_DTYPES = {
    "yaw_deg": np.float32, "gyro_z_dps": np.float32, "rpm": np.int16, "angle_sum": np.int64,
    "raw": np.int16, "z": np.float64, "valid": np.uint8, "kf6_rec": np.int32,
}


# elements per instance-tick of each input (fmskf_tick_inputs, include/fmskf.h)
_PER_TICK = {"yaw_deg": 1, "gyro_z_dps": 1, "rpm": 4, "angle_sum": 4, "raw": 8, "z": 8, "valid": 1,
             "kf6_rec": 4}


def kf6_records(yaw_deg, gyro_z_dps, rpm):
    """Pack KF6 inputs ([..., N] yaw and gyro, [..., N, 4] rpm; numpy or torch) into
    fmskf_kf6_record's: numpy -> [..., N] KF6_RECORD_DTYPE, torch -> [..., N, 4] int32."""
    if _is_torch(yaw_deg):
        import torch
        rec = torch.empty(tuple(yaw_deg.shape) + (4,), dtype=torch.int32, device=yaw_deg.device)
        rec[..., 0] = yaw_deg.view(torch.int32)
        rec[..., 1] = gyro_z_dps.view(torch.int32)
        rec[..., 2:] = rpm.contiguous().view(torch.int32)
        return rec
    rec = np.empty(np.shape(yaw_deg), KF6_RECORD_DTYPE)
    rec["yaw_deg"] = yaw_deg
    rec["gyro_z_dps"] = gyro_z_dps
    rec["rpm"] = rpm
    return rec


def pose_fix_records(robot, x, y, theta=None):
    """Pack absolute pose fixes ([count] robot indices, strictly ascending; x, y in metres,
    theta in radians or None; all numpy or all torch device tensors) into fmskf_pose_fix's:
    numpy -> [count] POSE_FIX_DTYPE, torch -> [count, 4] int32."""
    if _is_torch(robot):
        import torch
        rec = torch.zeros((robot.shape[0], 4), dtype=torch.int32, device=robot.device)
        rec[:, 0] = robot.to(torch.int32)  # the low 32 bits
        for k, v in ((1, x), (2, y), (3, theta)):
            if v is not None:
                rec[:, k] = v.to(torch.float32).contiguous().view(torch.int32)
        return rec
    rec = np.zeros(np.shape(robot), POSE_FIX_DTYPE)
    rec["robot"] = robot
    rec["x_m"] = x
    rec["y_m"] = y
    if theta is not None:
        rec["theta_rad"] = theta
    return rec


def range_fix_records(robot, anchor, range_m, var=None):
    """Pack measured ranges ([count] robot indices, non-descending; anchor indices into the
    handle's table; ranges in metres; var: each range's variance in m^2 or None for the call's
    default; all numpy or all torch device tensors) into fmskf_range_fix's: numpy -> [count]
    RANGE_FIX_DTYPE, torch -> [count, 4] int32."""
    if _is_torch(robot):
        import torch
        rec = torch.zeros((robot.shape[0], 4), dtype=torch.int32, device=robot.device)
        rec[:, 0] = robot.to(torch.int32)  # the low 32 bits
        rec[:, 1] = anchor.to(torch.int32)
        for k, v in ((2, range_m), (3, var)):
            if v is not None:
                rec[:, k] = v.to(torch.float32).contiguous().view(torch.int32)
        return rec
    rec = np.zeros(np.shape(robot), RANGE_FIX_DTYPE)
    rec["robot"] = robot
    rec["anchor"] = anchor
    rec["range_m"] = range_m
    if var is not None:
        rec["var_m2"] = var
    return rec


def _fix_noise(r):
    """packed lower triangle [6] of the 3x3 fix noise from a scalar variance, a diagonal [3],
    the packed triangle [6] or the matrix [3, 3]"""
    v = np.asarray(r, np.float64)
    if v.ndim == 0:
        v = np.full(3, float(v))
    if v.shape == (3, 3):
        return [v[i, j] for i in range(3) for j in range(i + 1)]
    if v.shape == (3,):
        return [v[0], 0.0, v[1], 0.0, 0.0, v[2]]
    if v.shape == (6,):
        return list(v)
    raise ValueError(f"fix noise: shape {v.shape}, want (), (3,), (6,) or (3, 3)")


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


class _Args:
    """Collects pointers of one call; all arrays must live in the same memory space."""

    def __init__(self):
        self.mem = None
        self.keep = []

    def ptr(self, a, dtype=None):
        if a is None:
            return None
        if _is_torch(a):
            if not a.is_cuda:
                a = a.numpy()
            else:
                if not a.is_contiguous():
                    raise ValueError("torch inputs must be contiguous")
                self._set(MEM_DEVICE)
                self.keep.append(a)
                return C.c_void_p(a.data_ptr())
        arr = np.ascontiguousarray(a, dtype=dtype) if dtype is not None else np.ascontiguousarray(a)
        self._set(MEM_HOST)
        self.keep.append(arr)
        return arr.ctypes.data_as(C.c_void_p)

    def _set(self, mem):
        if self.mem is None:
            self.mem = mem
        elif self.mem != mem:
            raise ValueError("mixing host and device arrays in one call")


class Engine:
    """Batched IMU + mecanum-odometry estimator over N robots on one GPU."""

    def __init__(self, model="kf6", n=1, device=0, trig=TRIG_TABLE512, dt=None, q=None, r=None,
                 p0=None, motor_dir=None, imu_read_reg=None, flags=0):
        L = load()
        self.model = MODEL_NAMES[model] if isinstance(model, str) else int(model)
        self.n = int(n)
        cfg = Config()
        check(L.fmskf_config_init(C.byref(cfg), self.model, self.n), "config_init")
        cfg.device = int(device)
        cfg.trig = int(trig)
        if dt is not None:
            cfg.dt = float(dt)
        for name, val in (("q", q), ("r", r), ("p0", p0)):
            if val is not None:
                dst = getattr(cfg, name)
                v = np.asarray(val, np.float64).ravel()
                for k in range(len(dst)):
                    dst[k] = float(v[k]) if k < v.size else 0.0
        if motor_dir is not None:
            for k in range(4):
                cfg.motor_dir[k] = int(motor_dir[k])
        if imu_read_reg is not None:
            cfg.imu_read_reg = int(imu_read_reg)
        cfg.flags = int(flags)  # FMSKF_CFG_* (CFG_COMP_POS: KF6 compensated positions)
        self.cfg = cfg
        h = C.c_void_p()
        check(L.fmskf_create(C.byref(cfg), C.byref(h)), "create")
        self.h = h
        nx, m, eb = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(L.fmskf_model_dims(self.model, C.byref(nx), C.byref(m), C.byref(eb)), "model_dims")
        self.nx, self.m, self.elem = nx.value, m.value, eb.value
        self.np_ = self.nx * (self.nx + 1) // 2
        self.dtype = np.float64 if self.elem == 8 else np.float32

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "h", None):
            load().fmskf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        check(load().fmskf_reset(self.h), "reset")

    def sync(self):
        check(load().fmskf_sync(self.h), "sync")

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream, a raw hipStream_t (int) or None (default stream)."""
        if stream is not None and hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        check(load().fmskf_set_stream(self.h, C.c_void_p(stream) if stream else None), "set_stream")

    def set_timing(self, enable=True):
        check(load().fmskf_set_timing(self.h, int(enable)), "set_timing")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        check(load().fmskf_last_kernel_ms(self.h, C.byref(ms)), "last_kernel_ms")
        return ms.value

    def kernel_time_total(self):
        """(sum of per-launch kernel times in ms, number of launches) since set_timing."""
        tot, cnt = C.c_double(), C.c_uint32()
        check(load().fmskf_kernel_time_total(self.h, C.byref(tot), C.byref(cnt)),
              "kernel_time_total")
        return tot.value, cnt.value

    # ------------------------------------------------------------------ ingest
    def ingest_wt901(self, data, lens, latch_qinit=False):
        """data: [N, stride] uint8 (one poll's UART bytes per robot), lens: [N] uint32."""
        a = _Args()
        stride = int(data.shape[1]) if hasattr(data, "shape") else 0
        pb = a.ptr(data, np.uint8)
        pl = a.ptr(lens, np.uint32)
        check(load().fmskf_ingest_wt901(self.h, pb, stride, pl, int(latch_qinit), a.mem),
              "ingest_wt901")

    def ingest_can(self, frames, stamps, present=None):
        """frames: [N, 4, 8] uint8, stamps: [N, 4] int16, present: [N] uint8 bitmask."""
        a = _Args()
        pf = a.ptr(frames, np.uint8)
        ps = a.ptr(stamps, np.int16)
        pp = a.ptr(present, np.uint8)
        check(load().fmskf_ingest_can(self.h, pf, ps, pp, a.mem), "ingest_can")

    # ------------------------------------------------------------------ innovation gate
    def set_gate(self, nis_max=None, max_consecutive=0):
        """fmskf_set_gate (KF6): reject a measurement whose normalized innovation squared exceeds
        nis_max (float('inf'): monitor only); after max_consecutive rejections in a row the next
        measurement is applied whatever its NIS (0: never).  nis_max=None turns the gate off."""
        if nis_max is None:
            check(load().fmskf_set_gate(self.h, None), "set_gate")
            return
        g = Gate(float(nis_max), int(max_consecutive))
        check(load().fmskf_set_gate(self.h, C.byref(g)), "set_gate")

    def get_gate(self):
        """fmskf_get_gate: dict of nis [N] float32, status [N] uint8 (GATE_NONE / ACCEPTED /
        REJECTED / FORCED), run [N] uint8 (consecutive rejections), rejects [N] uint32 (total)"""
        out = dict(nis=np.empty(self.n, np.float32), status=np.empty(self.n, np.uint8),
                   run=np.empty(self.n, np.uint8), rejects=np.empty(self.n, np.uint32))
        check(load().fmskf_get_gate(self.h, *(a.ctypes.data_as(C.c_void_p) for a in out.values()), MEM_HOST),
              "get_gate")
        return out

    # ------------------------------------------------------------------ per-row innovation gate
    def set_row_gate(self, d2_max=None, max_consecutive=0, record_d2=False):
        """fmskf_set_row_gate (EKF9, diagonal R): row a of the sequential update (heading, gyro z,
        ax, ay, vbx, vby) is skipped when its normalised innovation squared exceeds d2_max[a] (a
        scalar: the same threshold for every row; float('inf'): never); a row rejected
        max_consecutive times in a row is then applied whatever its d2 (0: never).  record_d2
        keeps every row's last d2 for get_row_gate.  d2_max=None turns the row gate off."""
        if d2_max is None:
            check(load().fmskf_set_row_gate(self.h, None), "set_row_gate")
            return
        g = RowGate()
        v = np.broadcast_to(np.asarray(d2_max, np.float32), (EKF9_ROWS,))
        for a in range(EKF9_ROWS):
            g.d2_max[a] = float(v[a])
        g.max_consecutive = int(max_consecutive)
        g.flags = ROW_GATE_D2 if record_d2 else 0
        check(load().fmskf_set_row_gate(self.h, C.byref(g)), "set_row_gate")
        self._row_d2 = bool(record_d2)

    def get_row_gate(self):
        """fmskf_get_row_gate: dict of status [6, N] uint8 (GATE_NONE / ACCEPTED / REJECTED /
        FORCED), run [6, N] uint8 (consecutive rejections) and, when the gate was set with
        record_d2, d2 [6, N] float32"""
        out = dict(status=np.empty((EKF9_ROWS, self.n), np.uint8), run=np.empty((EKF9_ROWS, self.n), np.uint8))
        if getattr(self, "_row_d2", False):
            out["d2"] = np.empty((EKF9_ROWS, self.n), np.float32)
        pd = out["d2"].ctypes.data_as(C.c_void_p) if "d2" in out else None
        check(load().fmskf_get_row_gate(self.h, out["status"].ctypes.data_as(C.c_void_p),
                                        out["run"].ctypes.data_as(C.c_void_p), pd, MEM_HOST), "get_row_gate")
        return out

    # ------------------------------------------------------------------ absolute pose fixes
    def correct_pose(self, robot=None, x=None, y=None, theta=None, r=1e-4, nis_max=float("inf"), out=False,
                     fixes=None, heading=None):
        """fmskf_correct_pose: fuse absolute fixes into the listed robots (KF6, EKF9).  `robot`
        [count] strictly ascending with x, y (and theta: the heading is then measured too), numpy
        arrays or torch device tensors; or `fixes`, records packed by pose_fix_records(), with `heading`
        saying whether theta_rad is read.  r: the fix noise (a variance, its diagonal [3], the
        packed triangle [6] or [3, 3]); nis_max: apply a fix only when its NIS <= nis_max.
        out=True returns (nis [count] float32, status [count] uint8: GATE_ACCEPTED / GATE_REJECTED
        / FIX_IGNORED) as numpy arrays (host list) or torch tensors (device list); out=(nis,
        status) writes into the given device tensors (a call that is captured)."""
        if fixes is None:
            fixes = pose_fix_records(robot, x, y, theta)
            if heading is None:
                heading = theta is not None
        prm = PoseFixParams()
        for k, v in enumerate(_fix_noise(r)):
            prm.r[k] = float(v)
        prm.nis_max = float(nis_max)
        prm.flags = FIX_HEADING if heading else 0
        a = _Args()
        if _is_torch(fixes):
            if str(fixes.dtype) != "torch.int32" or fixes.dim() != 2 or fixes.shape[1] != 4:
                raise TypeError("fixes: want a [count, 4] int32 tensor (pose_fix_records)")
            count = int(fixes.shape[0])
            pf = a.ptr(fixes)
        else:
            fixes = np.ascontiguousarray(fixes)
            if fixes.dtype != POSE_FIX_DTYPE:
                raise TypeError("fixes: want POSE_FIX_DTYPE records (pose_fix_records)")
            count = int(fixes.size)
            pf = a.ptr(fixes.view(np.uint32))
        mem = MEM_HOST if a.mem is None else a.mem
        nis = status = None
        if isinstance(out, tuple):
            nis, status = out
            if mem != MEM_DEVICE:
                raise TypeError("out tensors go with a device fix list")
        elif out and mem == MEM_DEVICE:
            import torch
            nis = torch.zeros(count, dtype=torch.float32, device=fixes.device)
            status = torch.zeros(count, dtype=torch.uint8, device=fixes.device)
        elif out:
            nis, status = np.zeros(count, np.float32), np.zeros(count, np.uint8)
        pn = a.ptr(nis) if nis is not None else None
        ps = a.ptr(status) if status is not None else None
        check(load().fmskf_correct_pose(self.h, pf, count, C.byref(prm), pn, ps, mem), "correct_pose")
        return (nis, status) if nis is not None or status is not None else None

    # ------------------------------------------------------------------ ranges against anchors
    def set_anchors(self, xyz):
        """fmskf_set_anchors: replace the handle's anchor table with xyz [count, 3] (metres; a
        host array); an empty array clears it."""
        a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        check(load().fmskf_set_anchors(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0]), "set_anchors")

    def get_anchors(self):
        """fmskf_get_anchors: the anchor table, [count, 3] float32"""
        out = np.zeros((RANGE_ANCHORS_MAX, 3), np.float32)
        cnt = C.c_uint32()
        check(load().fmskf_get_anchors(self.h, out.ctypes.data_as(C.c_void_p), RANGE_ANCHORS_MAX, C.byref(cnt)),
              "get_anchors")
        return out[:cnt.value].copy()

    def correct_range(self, robot=None, anchor=None, range_m=None, var=None, *, fixes=None, tag=(0.0, 0.0, 0.0),
                      var_default, d2_max=float("inf"), d_min, out=False):
        """fmskf_correct_range: fuse measured ranges to the anchors of set_anchors() into the
        listed robots (KF6, EKF9).  `robot` [count] non-descending (the consecutive entries of one
        robot, a burst, are applied in order) with anchor, range_m and optionally var (per-range
        variances; entries <= 0 take var_default), numpy arrays or torch device tensors; or `fixes`,
        records packed by range_fix_records().  tag: the antenna (lx, ly in the body frame, lz its
        height); d2_max: apply a range only when its normalised innovation squared <= d2_max;
        d_min: below this predicted distance nothing is done (RANGE_NEAR).  out=True returns (d2
        [count] float32, status [count] uint8: GATE_ACCEPTED / GATE_REJECTED / RANGE_NEAR /
        FIX_IGNORED) as numpy arrays (host list) or torch tensors (device list); out=(d2, status)
        writes into the given device tensors (a call that is captured)."""
        if fixes is None:
            fixes = range_fix_records(robot, anchor, range_m, var)
        prm = RangeParams()
        for k in range(3):
            prm.tag[k] = float(tag[k])
        prm.var_m2 = float(var_default)
        prm.d2_max = float(d2_max)
        prm.d_min = float(d_min)
        a = _Args()
        if _is_torch(fixes):
            if str(fixes.dtype) != "torch.int32" or fixes.dim() != 2 or fixes.shape[1] != 4:
                raise TypeError("fixes: want a [count, 4] int32 tensor (range_fix_records)")
            count = int(fixes.shape[0])
            pf = a.ptr(fixes)
        else:
            fixes = np.ascontiguousarray(fixes)
            if fixes.dtype != RANGE_FIX_DTYPE:
                raise TypeError("fixes: want RANGE_FIX_DTYPE records (range_fix_records)")
            count = int(fixes.size)
            pf = a.ptr(fixes.view(np.uint32))
        mem = MEM_HOST if a.mem is None else a.mem
        d2 = status = None
        if isinstance(out, tuple):
            d2, status = out
            if mem != MEM_DEVICE:
                raise TypeError("out tensors go with a device range list")
        elif out and mem == MEM_DEVICE:
            import torch
            d2 = torch.zeros(count, dtype=torch.float32, device=fixes.device)
            status = torch.zeros(count, dtype=torch.uint8, device=fixes.device)
        elif out:
            d2, status = np.zeros(count, np.float32), np.zeros(count, np.uint8)
        pd = a.ptr(d2) if d2 is not None else None
        ps = a.ptr(status) if status is not None else None
        check(load().fmskf_correct_range(self.h, pf, count, C.byref(prm), pd, ps, mem), "correct_range")
        return (d2, status) if d2 is not None or status is not None else None

    # ------------------------------------------------------------------ selection, listed robots
    def select(self, nonfinite=False, pos_var_min=None, gate_run_min=None, row_mask=None, capacity=None,
               out=None):
        """fmskf_select: the robots (ascending) for which any requested criterion holds --
        nonfinite: a NaN / Inf in x or P; pos_var_min: P[0][0] + P[1][1] > pos_var_min;
        gate_run_min: consecutive gate rejections >= gate_run_min (KF6 with set_gate; EKF9 with
        set_row_gate, over the rows of row_mask, default all six).  Returns (robots, reason, count):
        count the number of matches (never capped), reason[k] the SEL_* bits that held for
        robots[k].
        out=None: numpy arrays trimmed to min(count, capacity) entries (capacity: default N; 0: a
        count-only call).  out=(robots, reason): the caller's arrays of `capacity` entries (default:
        their length), written up to min(count, capacity) and returned whole; reason may be None.
        Host: uint32 / uint8 numpy arrays, count comes back as an int.  Device: int32 / uint8
        torch tensors with an optional third, an int64 [1] tensor that receives the count (made
        when absent); the call is then asynchronous on the handle's stream."""
        prm = SelectParams()
        prm.criteria = (SEL_NONFINITE if nonfinite else 0) | (SEL_POS_VAR if pos_var_min is not None else 0) | \
            (SEL_GATE_RUN if gate_run_min is not None else 0)
        prm.pos_var_min = float(pos_var_min) if pos_var_min is not None else 0.0
        prm.run_min = int(gate_run_min) if gate_run_min is not None else 0
        if row_mask is None:
            row_mask = 0x3F if gate_run_min is not None and self.model == MODEL_EKF9 else 0
        prm.row_mask = int(row_mask)
        fn = load().fmskf_select
        if out is None:
            cap = self.n if capacity is None else int(capacity)
            robots = np.empty(cap, np.uint32)
            reason = np.empty(cap, np.uint8)
            cnt = C.c_uint64()
            check(fn(self.h, C.byref(prm), robots.ctypes.data_as(C.c_void_p) if cap else None,
                     reason.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(cnt), MEM_HOST), "select")
            got = min(cnt.value, cap)
            return robots[:got], reason[:got], cnt.value
        robots, reason = out[0], out[1]
        if _is_torch(robots):
            import torch
            cnt = out[2] if len(out) > 2 else torch.zeros(1, dtype=torch.int64, device=robots.device)
            for name, t, dt in (("robots", robots, "int32"), ("reason", reason, "uint8"), ("count", cnt, "int64")):
                if t is not None and not (t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch." + dt):
                    raise TypeError(f"select: {name} must be a contiguous {dt} device tensor")
            cap = int(robots.numel()) if capacity is None else int(capacity)
            if cap > robots.numel() or (reason is not None and cap > reason.numel()) or cnt.numel() < 1:
                raise ValueError("select: capacity above the length of the out tensors")
            check(fn(self.h, C.byref(prm), C.c_void_p(robots.data_ptr()),
                     C.c_void_p(reason.data_ptr()) if reason is not None else None, cap,
                     C.c_void_p(cnt.data_ptr()), MEM_DEVICE), "select")
            return robots, reason, cnt
        for name, a, dt in (("robots", robots, np.uint32), ("reason", reason, np.uint8)):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous
                                      and a.flags.writeable):
                raise TypeError(f"select: {name} must be a writable C-contiguous {np.dtype(dt).name} numpy array")
        cap = (0 if robots is None else robots.size) if capacity is None else int(capacity)
        if (cap and robots is None) or (robots is not None and cap > robots.size) or \
                (reason is not None and cap > reason.size):
            raise ValueError("select: capacity above the length of the out arrays")
        cnt = C.c_uint64()
        check(fn(self.h, C.byref(prm), robots.ctypes.data_as(C.c_void_p) if robots is not None else None,
                 reason.ctypes.data_as(C.c_void_p) if reason is not None else None, cap, C.byref(cnt), MEM_HOST),
              "select")
        return robots, reason, cnt.value

    def _lo_rows(self):
        rows = C.c_uint32()
        check(load().fmskf_get_state_lo(self.h, None, C.byref(rows), MEM_HOST), "get_state_lo")
        return rows.value

    def _robot_list(self, a, robots, what):
        """(pointer, count) of a robot list: a uint32 numpy array (host) or an int32 device tensor"""
        if _is_torch(robots) and robots.is_cuda:
            if str(robots.dtype) != "torch.int32" or robots.dim() != 1:
                raise TypeError(f"{what}: a device robot list must be a 1-d int32 tensor")
            return a.ptr(robots), int(robots.numel())
        robots = np.ascontiguousarray(robots)
        if robots.ndim != 1 or robots.dtype.kind not in "iu":
            raise TypeError(f"{what}: robots must be a 1-d integer array")
        if robots.size and (robots.min() < 0 or robots.max() > 0xFFFFFFFF):
            raise ValueError(f"{what}: robot index out of the uint32 range")
        return a.ptr(robots, np.uint32), int(robots.size)

    def get_state_subset(self, robots):
        """fmskf_get_state_subset: (x [n, count], P [n(n+1)/2, count], lo [rows, count] or None
        when the model keeps no low parts) of the listed robots -- strictly ascending; a uint32
        numpy array (numpy results) or an int32 device tensor (torch device results, asynchronous
        on the handle's stream)."""
        a = _Args()
        pr, count = self._robot_list(a, robots, "get_state_subset")
        rows = self._lo_rows()
        if a.mem == MEM_DEVICE:
            import torch
            mk = lambda r: torch.empty((r, count), dtype=torch.float32, device=robots.device)
        else:
            mk = lambda r: np.empty((r, count), np.float32)
        x, P, lo = mk(self.nx), mk(self.np_), (mk(rows) if rows else None)
        check(load().fmskf_get_state_subset(self.h, pr, count, a.ptr(x), a.ptr(P),
                                            a.ptr(lo) if lo is not None else None, a.mem), "get_state_subset")
        return x, P, lo

    def get_state_subset_into(self, robots, x=None, P=None, lo=None):
        """fmskf_get_state_subset into the caller's arrays ([rows, count] float32, in the list's
        memory space; None skips an array): the form a graph capture takes"""
        a = _Args()
        pr, count = self._robot_list(a, robots, "get_state_subset")
        ps = self._subset_planes(a, count, x, P, lo, "get_state_subset")
        check(load().fmskf_get_state_subset(self.h, pr, count, *ps, a.mem), "get_state_subset")

    def _subset_planes(self, a, count, x, P, lo, what):
        out = []
        for name, v, rows in (("x", x, self.nx), ("P", P, self.np_), ("lo", lo, None)):
            if v is not None:
                if _is_torch(v) and v.is_cuda and str(v.dtype) != "torch.float32":
                    raise TypeError(f"{what}: {name} must be float32")
                if len(v.shape) != 2 or v.shape[1] != count or (rows is not None and v.shape[0] != rows):
                    raise ValueError(f"{what}: {name} has shape {tuple(v.shape)}, want [{rows or 'rows'}, {count}]")
            out.append(a.ptr(v, np.float32) if v is not None else None)
        rows = self._lo_rows() if lo is not None else 0
        if rows and lo.shape[0] != rows:  # a model without low rows: the library refuses lo
            raise ValueError(f"{what}: lo has {lo.shape[0]} rows, the model keeps {rows}")
        return out

    def set_state_subset(self, robots, x=None, P=None, lo=None):
        """fmskf_set_state_subset: overwrite the listed robots' state with the columns of x
        [n, count], P [n(n+1)/2, count], lo [rows, count] (any may be None), leaving every other
        robot alone.  A given x restarts the heading low part, with CFG_COMP_POS a given x or P the
        position low parts, unless lo is given.  The list and the arrays are all numpy (host) or
        all torch device tensors (asynchronous; the form a graph capture takes)."""
        a = _Args()
        pr, count = self._robot_list(a, robots, "set_state_subset")
        ps = self._subset_planes(a, count, x, P, lo, "set_state_subset")
        check(load().fmskf_set_state_subset(self.h, pr, count, *ps, a.mem), "set_state_subset")

    # ------------------------------------------------------------------ ticks
    def _inputs(self, kw, n_ticks=1, stride=None):
        a = _Args()
        ti = TickInputs()
        unknown = set(kw) - set(_PER_TICK)
        if unknown:
            raise TypeError(f"unknown tick inputs: {sorted(unknown)}")
        stride = self.n if stride is None else stride
        for name in ("yaw_deg", "gyro_z_dps", "rpm", "angle_sum", "raw", "z", "valid", "kf6_rec"):
            v = kw.get(name)
            if name == "kf6_rec" and isinstance(v, np.ndarray) and v.dtype.names:
                v = np.ascontiguousarray(v).view(np.int32)
            if v is not None:
                # the C ABI takes bare pointers: check extents here, before the kernel reads
                need = ((int(n_ticks) - 1) * int(stride) + self.n) * _PER_TICK[name]
                nd = v.dim() if _is_torch(v) else np.ndim(v)
                if name == "angle_sum" and n_ticks == 1 and nd == 2 and v.shape[0] == 4 \
                        and v.shape[1] > self.n:
                    ti.angle_sum_pitch = int(v.shape[1])  # padded [4][pitch] planes
                    need = 3 * int(v.shape[1]) + self.n
                have = v.numel() if _is_torch(v) else np.size(v)
                if have < need:
                    raise ValueError(f"{name}: {have} elements, {n_ticks} tick(s) need {need}")
                if _is_torch(v) and v.is_cuda and str(v.dtype) != "torch." + np.dtype(_DTYPES[name]).name:
                    raise TypeError(f"{name}: dtype {v.dtype}, expected {np.dtype(_DTYPES[name]).name}")
            p = a.ptr(v, _DTYPES[name])
            setattr(ti, name, p.value if p is not None else None)
        ti.mem = MEM_HOST if a.mem is None else a.mem
        return ti, a

    def correct(self, **kw):
        ti, _keep = self._inputs(kw)
        check(load().fmskf_correct(self.h, C.byref(ti)), "correct")

    def predict(self, **kw):
        ti, _keep = self._inputs(kw)
        check(load().fmskf_predict(self.h, C.byref(ti)), "predict")

    def tick(self, **kw):
        ti, _keep = self._inputs(kw)
        check(load().fmskf_tick(self.h, C.byref(ti)), "tick")

    def prepare(self, **kw):
        """Pre-built fmskf_tick_inputs for a hot loop: returns an opaque object to pass to
        tick_prepared() (keeps the arrays alive)."""
        ti, keep = self._inputs(kw)
        return (ti, keep, C.byref(ti))

    def tick_prepared(self, prepared, _tick=None):
        rc = (_tick or load().fmskf_tick)(self.h, prepared[2])
        if rc:
            check(rc, "tick")

    def tick_many(self, n_ticks, tick_stride=None, **kw):
        stride = self.n if tick_stride is None else int(tick_stride)
        ti, _keep = self._inputs(kw, n_ticks, stride)
        check(load().fmskf_tick_many(self.h, C.byref(ti), int(n_ticks), stride), "tick_many")

    def tick_many_smooth(self, n_ticks, tick_stride=None, want_P=False, out_x=None, out_P=None, pitch=0, **kw):
        """fmskf_tick_many_smooth (KF6): the ticks of tick_many, plus the fixed-interval
        (Rauch-Tung-Striebel) smoothed state of every tick, x_s [T, 6, N], and with want_P (or
        out_P) its covariance, P_s [T, 21, N] packed like get_state.  Returns x_s, or (x_s, P_s).
        numpy inputs give numpy results; torch device inputs give torch device results,
        asynchronous on the handle's stream.  out_x / out_P: the caller's C-contiguous float32
        arrays [T, 6, pitch or N] / [T, 21, pitch or N] (numpy, or torch device tensors whatever
        the inputs' memory); with pitch > N the elements past N of every row are left alone."""
        T = int(n_ticks)
        stride = self.n if tick_stride is None else int(tick_stride)
        ti, keep = self._inputs(kw, T, stride)
        cols = int(pitch) if pitch else self.n
        if out_x is None and out_P is not None:
            raise ValueError("tick_many_smooth: out_P without out_x")
        want_P = bool(want_P) or out_P is not None
        if out_x is None:
            if keep.mem == MEM_DEVICE:
                import torch
                dev = keep.keep[0].device
                mk = lambda r: torch.empty((T, r, cols), dtype=torch.float32, device=dev)
            else:
                mk = lambda r: np.empty((T, r, cols), np.float32)
            out_x = mk(self.nx)
        if want_P and out_P is None:
            if _is_torch(out_x):
                import torch
                out_P = torch.empty((T, self.np_, cols), dtype=torch.float32, device=out_x.device)
            else:
                out_P = np.empty((T, self.np_, cols), np.float32)
        so = _lib.SmoothOut()
        for name, v, rows in (("out_x", out_x, self.nx), ("out_P", out_P, self.np_)):
            if v is None:
                continue
            if tuple(v.shape) != (T, rows, cols):
                raise ValueError(f"tick_many_smooth: {name} has shape {tuple(v.shape)}, want {(T, rows, cols)}")
            if _is_torch(v):
                if not v.is_cuda or not v.is_contiguous() or str(v.dtype) != "torch.float32":
                    raise TypeError(f"tick_many_smooth: a torch {name} must be a contiguous float32 device tensor")
            elif not isinstance(v, np.ndarray) or v.dtype != np.float32 or not v.flags.c_contiguous \
                    or not v.flags.writeable:
                raise TypeError(f"tick_many_smooth: a host {name} must be a writable C-contiguous float32 numpy array")
        if out_P is not None and _is_torch(out_P) != _is_torch(out_x):
            raise ValueError("tick_many_smooth: out_x and out_P must live in the same memory")
        ptr = (lambda v: v.data_ptr()) if _is_torch(out_x) else (lambda v: v.ctypes.data)
        so.mem = MEM_DEVICE if _is_torch(out_x) else MEM_HOST
        so.pitch = int(pitch)
        so.x = ptr(out_x)
        so.P = ptr(out_P) if out_P is not None else None
        check(load().fmskf_tick_many_smooth(self.h, C.byref(ti), T, stride, C.byref(so)), "tick_many_smooth")
        return (out_x, out_P) if want_P else out_x

    def smooth_workspace_bytes(self, n_ticks) -> int:
        """fmskf_smooth_workspace_bytes: the history tick_many_smooth keeps for a window of n_ticks"""
        b = C.c_uint64()
        check(load().fmskf_smooth_workspace_bytes(self.h, int(n_ticks), C.byref(b)), "smooth_workspace_bytes")
        return b.value

    def smooth_reserve(self, n_ticks):
        """fmskf_smooth_reserve: allocate the history of a window of n_ticks ahead of time (it only
        grows); 0 frees it"""
        check(load().fmskf_smooth_reserve(self.h, int(n_ticks)), "smooth_reserve")

    def _window_out(self, call, shapes, planes, st, flag, names, accumulate_into, keep):
        """The output dict of tick_many_loglik / tick_many_em and its ctypes struct `st`, filled: new
        arrays for `names` in the memory of the inputs (keep), or the caller's accumulate_into
        (validated; `flag` set).  shapes: every key the call knows; planes: its multi-row keys, which
        share one row pitch >= N."""
        if accumulate_into is None:
            if keep.mem == MEM_DEVICE:
                import torch
                dev = keep.keep[0].device
                mk = lambda k: torch.empty(shapes[k], dtype=torch.int32 if k == "n_meas" else torch.float64, device=dev)
            else:
                mk = lambda k: np.empty(shapes[k], np.uint32 if k == "n_meas" else np.float64)
            out = {k: mk(k) for k in names}
        else:
            out = accumulate_into
            st.flags = flag
            if not out or set(out) - set(shapes):
                raise ValueError(f"{call}: accumulate_into needs some of {sorted(shapes)} and nothing else")
        tor = [_is_torch(v) for v in out.values()]
        if any(tor) != all(tor):
            raise ValueError(f"{call}: the outputs must live in the same memory")
        cols = {int(out[k].shape[-1]) for k in planes if k in out and len(out[k].shape) == 2}
        if len(cols) > 1 or (cols and min(cols) < self.n):
            raise ValueError(f"{call}: {' and '.join(planes)} need one row pitch >= N")
        pitch = cols.pop() if cols else self.n
        for k, v in out.items():
            want = shapes[k] if len(shapes[k]) == 1 else (shapes[k][0], pitch)
            if tuple(v.shape) != want:
                raise ValueError(f"{call}: {k} has shape {tuple(v.shape)}, want {want}")
            if tor[0]:
                dt = "torch.float64" if k != "n_meas" else None
                if not v.is_cuda or not v.is_contiguous() or (str(v.dtype) != dt if dt else v.element_size() != 4):
                    raise TypeError(f"{call}: a torch {k} must be a contiguous device tensor of "
                                    f"{'float64' if dt else 'int32'}")
            elif not isinstance(v, np.ndarray) or v.dtype != (np.uint32 if k == "n_meas" else np.float64) \
                    or not v.flags.c_contiguous or not v.flags.writeable:
                raise TypeError(f"{call}: a host {k} must be a writable C-contiguous numpy array of "
                                f"{'uint32' if k == 'n_meas' else 'float64'}")
            setattr(st, k, v.data_ptr() if tor[0] else v.ctypes.data)
        st.mem = MEM_DEVICE if tor[0] else MEM_HOST
        st.pitch = 0 if pitch == self.n else pitch
        return out, st

    def tick_many_loglik(self, n_ticks, tick_stride=None, moments=False, total=False, accumulate_into=None, **kw):
        """fmskf_tick_many_loglik (KF6): the ticks of tick_many, plus the window's innovation sums
        per robot.  Returns a dict: n_meas [N] uint32, nis_sum [N] and logdet_sum [N] float64 (what
        fmskf.loglik takes); with moments innov_sum [4, N] and innov_outer [10, N] (the sums of y
        and of y y^T, packed lower triangle); with total the fleet's total [4] = sum n_meas, sum
        nis_sum, sum logdet_sum, robots left out.  numpy inputs give numpy results; torch device
        inputs give torch device results, asynchronous on the handle's stream.
        accumulate_into: a dict of such arrays (an earlier call's result: a log replayed in chunks);
        this call's sums are added to them (FMSKF_LL_ACCUMULATE) and the same arrays returned.  Its
        keys select the outputs, its memory is the results' memory, and innovation planes wider
        than N (a padded pitch) keep their elements past N."""
        T = int(n_ticks)
        stride = self.n if tick_stride is None else int(tick_stride)
        ti, keep = self._inputs(kw, T, stride)
        shapes = {"n_meas": (self.n,), "nis_sum": (self.n,), "logdet_sum": (self.n,), "innov_sum": (4, self.n),
                  "innov_outer": (10, self.n), "total": (4,)}
        names = ["n_meas", "nis_sum", "logdet_sum"] + (["innov_sum", "innov_outer"] if moments else []) + \
            (["total"] if total else [])
        out, lo = self._window_out("tick_many_loglik", shapes, ("innov_sum", "innov_outer"), _lib.LoglikOut(),
                                   _lib.LL_ACCUMULATE, names, accumulate_into, keep)
        check(load().fmskf_tick_many_loglik(self.h, C.byref(ti), T, stride, C.byref(lo)), "tick_many_loglik")
        return out

    def tick_many_em(self, n_ticks, tick_stride=None, per_robot=False, total=True, accumulate_into=None, **kw):
        """fmskf_tick_many_em (KF6): the ticks of tick_many, plus the EM sufficient statistics for Q
        and R of the smoothed window.  Returns a dict: with total the fleet's total [34] = sum
        n_trans, sum n_meas, robots left out, sq [21], sr [10] (what fmskf.em_mstep takes); with
        per_robot n_meas [N] uint32, sq [21, N] and sr [10, N] float64 (packed lower triangles).
        numpy inputs give numpy results; torch device inputs give torch device results,
        asynchronous on the handle's stream.
        accumulate_into: a dict of such arrays (an earlier call's result: another window, another
        log); this call's sums are added to them (FMSKF_EM_ACCUMULATE) and the same arrays
        returned.  Its keys select the outputs, its memory is the results' memory, and sq / sr
        planes wider than N (a padded pitch) keep their elements past N.  Every call smooths its
        own window: the transition between two windows is not a term."""
        T = int(n_ticks)
        stride = self.n if tick_stride is None else int(tick_stride)
        ti, keep = self._inputs(kw, T, stride)
        shapes = {"n_meas": (self.n,), "sq": (21, self.n), "sr": (10, self.n), "total": (_lib.EM_TOTAL_LEN,)}
        names = (["n_meas", "sq", "sr"] if per_robot else []) + (["total"] if total else [])
        if accumulate_into is None and not names:
            raise ValueError("tick_many_em: neither per_robot nor total")
        out, eo = self._window_out("tick_many_em", shapes, ("sq", "sr"), _lib.EmOut(), _lib.EM_ACCUMULATE, names,
                                   accumulate_into, keep)
        check(load().fmskf_tick_many_em(self.h, C.byref(ti), T, stride, C.byref(eo)), "tick_many_em")
        return out

    def tick_many_trace(self, n_ticks, tick_stride=None, every=None, want_P=False, pitch=0, out=None, **kw):
        """fmskf_tick_many_trace (KF6, with or without a gate): the ticks of tick_many, plus what the
        filter did at every tick.  Returns a dict of the planes asked for: nis [T, C] float32 (the
        quiet NaN 0x7FC00000 where the tick carried no measurement), status [T, C] uint8 (GATE_*),
        applied [T, C] uint8 (1 where the update ran: the format of `valid` with tick_stride == C);
        with `every` x [T // every, 6, C], the state after ticks every, 2 * every, ..., and with
        want_P (every defaults to 1 then) P [T // every, 21, C] packed like get_state.  C = pitch,
        or N; with pitch > N the elements past N of every row are left alone.  numpy inputs give
        numpy results; torch device inputs give torch device results, asynchronous on the
        handle's stream.
        out: a dict of the caller's arrays instead (some of nis, status, applied, x, P; numpy, or
        contiguous torch device tensors whatever the inputs' memory); its keys select the outputs,
        an array may have more rows than the call writes, and those are left alone."""
        T = int(n_ticks)
        stride = self.n if tick_stride is None else int(tick_stride)
        ti, keep = self._inputs(kw, T, stride)
        cols = int(pitch) if pitch else self.n
        if cols < self.n:
            raise ValueError("tick_many_trace: pitch < N")
        dts = {"nis": np.float32, "status": np.uint8, "applied": np.uint8, "x": np.float32, "P": np.float32}
        if out is None:
            if want_P and every is None:
                every = 1
            names = ["nis", "status", "applied"] + (["x"] if every is not None else []) + (["P"] if want_P else [])
        else:
            names = list(out)
            if not names or set(names) - set(dts):
                raise ValueError(f"tick_many_trace: out needs some of {sorted(dts)} and nothing else")
            if every is None and ("x" in out or "P" in out):
                every = 1
        ev = 0 if every is None else int(every)
        if ("x" in names or "P" in names) and not 1 <= ev <= T:
            raise ValueError("tick_many_trace: every must be 1 .. n_ticks")
        rows = T // ev if ev else 0
        shapes = {"nis": (T, cols), "status": (T, cols), "applied": (T, cols), "x": (rows, self.nx, cols),
                  "P": (rows, self.np_, cols)}
        if out is None:
            if keep.mem == MEM_DEVICE:
                import torch
                dev = keep.keep[0].device
                out = {k: torch.empty(shapes[k], dtype=getattr(torch, np.dtype(dts[k]).name), device=dev) for k in names}
            else:
                out = {k: np.empty(shapes[k], dts[k]) for k in names}
        tor = [_is_torch(v) for v in out.values()]
        if any(tor) != all(tor):
            raise ValueError("tick_many_trace: the outputs must live in the same memory")
        to = _lib.TraceOut()
        for k, v in out.items():
            want = shapes[k]
            if len(v.shape) != len(want) or v.shape[0] < want[0] or tuple(v.shape[1:]) != want[1:]:
                raise ValueError(f"tick_many_trace: {k} has shape {tuple(v.shape)}, want {want} (or more rows)")
            name = np.dtype(dts[k]).name
            if tor[0]:
                if not v.is_cuda or not v.is_contiguous() or str(v.dtype) != "torch." + name:
                    raise TypeError(f"tick_many_trace: a torch {k} must be a contiguous {name} device tensor")
            elif not isinstance(v, np.ndarray) or v.dtype != dts[k] or not v.flags.c_contiguous or not v.flags.writeable:
                raise TypeError(f"tick_many_trace: a host {k} must be a writable C-contiguous {name} numpy array")
            setattr(to, k, v.data_ptr() if tor[0] else v.ctypes.data)
        to.mem = MEM_DEVICE if tor[0] else MEM_HOST
        to.pitch = 0 if cols == self.n else cols
        to.every = ev
        check(load().fmskf_tick_many_trace(self.h, C.byref(ti), T, stride, C.byref(to)), "tick_many_trace")
        return out

    # ------------------------------------------------------------------ readout
    def get_state(self):
        x = np.empty((self.nx, self.n), self.dtype)
        P = np.empty((self.np_, self.n), self.dtype) if self.m else None
        check(load().fmskf_get_state(self.h, x.ctypes.data_as(C.c_void_p),
                                     P.ctypes.data_as(C.c_void_p) if P is not None else None,
                                     MEM_HOST), "get_state")
        return x, P

    def set_state(self, x, P=None):
        a = _Args()
        px = a.ptr(x, self.dtype)
        pP = a.ptr(P, self.dtype) if P is not None else None
        check(load().fmskf_set_state(self.h, px, pP, a.mem), "set_state")

    def get_state_lo(self):
        """the hidden low-part rows [rows][N] float32 (EKF9: the heading; KF6 with CFG_COMP_POS:
        px, py, P00, P10, P11), or None when the model keeps none"""
        rows = C.c_uint32()
        check(load().fmskf_get_state_lo(self.h, None, C.byref(rows), MEM_HOST), "get_state_lo")
        if rows.value == 0:
            return None
        lo = np.empty((rows.value, self.n), np.float32)
        check(load().fmskf_get_state_lo(self.h, lo.ctypes.data_as(C.c_void_p), C.byref(rows), MEM_HOST),
              "get_state_lo")
        return lo

    def set_state_lo(self, lo):
        """restore the hidden low-part rows: `lo` must be [rows][N] float32 (host or device),
        rows as get_state_lo returns them"""
        if lo is None:
            raise ValueError("set_state_lo: lo is None")
        rows = C.c_uint32()
        check(load().fmskf_get_state_lo(self.h, None, C.byref(rows), MEM_HOST), "get_state_lo")
        if rows.value == 0:
            raise FmskfError(ENOTSUP, "set_state_lo", "this model keeps no low-part rows")
        want = (rows.value, self.n)
        if tuple(lo.shape) != want:
            raise ValueError(f"set_state_lo: shape {tuple(lo.shape)}, want {want}")
        if _is_torch(lo):
            import torch
            if lo.dtype != torch.float32:
                raise ValueError(f"set_state_lo: dtype {lo.dtype}, want float32")
        elif np.asarray(lo).dtype != np.float32:
            raise ValueError(f"set_state_lo: dtype {np.asarray(lo).dtype}, want float32")
        a = _Args()
        check(load().fmskf_set_state_lo(self.h, a.ptr(lo, np.float32), a.mem), "set_state_lo")

    def save_state(self, path):
        """fmskf_save_state: checkpoint every per-robot array of the handle to `path`"""
        check(load().fmskf_save_state(self.h, str(path).encode()), "save_state")

    def load_state(self, path):
        """fmskf_load_state: resume from a checkpoint of a handle of the same model and N"""
        check(load().fmskf_load_state(self.h, str(path).encode()), "load_state")

    def _planes3(self, fn, what, out, planes):
        """a readout of three [N] float planes into `out` [3, N] float32: None (a new numpy
        array), a C-contiguous numpy array (host) or a contiguous torch CUDA tensor (device, on
        the handle's stream, no host wait).  planes[k] False passes NULL for plane k, whose row
        of `out` is left as it is (zero in a new array)."""
        planes = tuple(bool(p) for p in planes)
        if len(planes) != 3:
            raise ValueError(f"{what}: planes wants three flags")
        if out is None:
            out = np.empty((3, self.n), np.float32) if all(planes) else np.zeros((3, self.n), np.float32)
        if tuple(out.shape) != (3, self.n):
            raise ValueError(f"{what}: out shape {tuple(out.shape)}, want {(3, self.n)}")
        if _is_torch(out):
            if not out.is_cuda or not out.is_contiguous() or str(out.dtype) != "torch.float32":
                raise TypeError(f"{what}: a torch `out` must be a contiguous float32 CUDA tensor")
            p = [C.c_void_p(out[k].data_ptr()) if planes[k] else None for k in range(3)]
            mem = MEM_DEVICE
        else:
            if not isinstance(out, np.ndarray) or out.dtype != np.float32 or not out.flags.c_contiguous \
                    or not out.flags.writeable:
                raise TypeError(f"{what}: a host `out` must be a writable C-contiguous float32 numpy array")
            p = [out[k].ctypes.data_as(C.c_void_p) if planes[k] else None for k in range(3)]
            mem = MEM_HOST
        check(fn(self.h, *p, mem), what)
        return out

    def get_pose(self, out=None, planes=(True, True, True)):
        """fmskf_get_pose: [3, N] float32 (x m, y m, th rad); `out`, `planes` as _planes3"""
        return self._planes3(load().fmskf_get_pose, "get_pose", out, planes)

    def get_vel(self, out=None, planes=(True, True, True)):
        """fmskf_get_vel: [3, N] float32 (body vx mm/s, vy mm/s, vth rad/s); `out`, `planes` as
        _planes3"""
        return self._planes3(load().fmskf_get_vel, "get_vel", out, planes)

    def get_prev_sum(self):
        out = np.empty((4, self.n), np.int64)
        check(load().fmskf_get_prev_sum(self.h, out.ctypes.data_as(C.c_void_p), MEM_HOST),
              "get_prev_sum")
        return out

    def get_imu(self):
        data = np.empty((16, self.n), np.float32)
        err = np.empty(self.n, np.uint8)
        check(load().fmskf_get_imu(self.h, data.ctypes.data_as(C.c_void_p),
                                   err.ctypes.data_as(C.c_void_p), MEM_HOST), "get_imu")
        return data, err

    def get_imu_regs(self):
        regs = np.empty((0x90, self.n), np.int16)
        pend = np.empty(self.n, np.uint8)
        check(load().fmskf_get_imu_regs(self.h, regs.ctypes.data_as(C.c_void_p),
                                        pend.ctypes.data_as(C.c_void_p), MEM_HOST), "get_imu_regs")
        return regs, pend

    def get_motors(self):
        ang = np.empty((self.n, 4), np.int16)
        rpm = np.empty((self.n, 4), np.int16)
        cur = np.empty((self.n, 4), np.int16)
        s = np.empty((4, self.n), np.int64)
        spd = np.empty((4, self.n), np.float32)
        check(load().fmskf_get_motors(self.h, *(a.ctypes.data_as(C.c_void_p)
                                                for a in (ang, rpm, cur, s, spd)), MEM_HOST),
              "get_motors")
        return dict(angle=ang, rpm=rpm, curr=cur, angle_sum=s, speed_radps=spd)

    def get_motor_status(self):
        """MOTOR_IF_M2006::get_status_latest of every wheel: [N][4] each of s16_microsec_id,
        s16_rawAngle, s16_rawSpeedRpm, s16_rawCurr, flt_dltOutAngle_rad, flt_SpeedRadPS"""
        out = dict(microsec_id=np.empty((self.n, 4), np.int16), angle=np.empty((self.n, 4), np.int16),
                   rpm=np.empty((self.n, 4), np.int16), curr=np.empty((self.n, 4), np.int16),
                   dlt_out_angle_rad=np.empty((self.n, 4), np.float32),
                   speed_radps=np.empty((self.n, 4), np.float32))
        check(load().fmskf_get_motor_status(self.h, *(a.ctypes.data_as(C.c_void_p) for a in out.values()),
                                            MEM_HOST), "get_motor_status")
        return out

    # ------------------------------------------------------------------ HIP graph
    def graph_begin(self):
        check(load().fmskf_graph_begin(self.h), "graph_begin")

    def graph_end(self):
        check(load().fmskf_graph_end(self.h), "graph_end")

    def graph_launch(self, times=1):
        check(load().fmskf_graph_launch(self.h, int(times)), "graph_launch")

    # ------------------------------------------------------------------ native RCCL path
    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """fmskf_comm_init: an RCCL communicator owned by this handle (one process per GPU)"""
        b = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        check(load().fmskf_comm_init(self.h, b, int(rank), int(world)), "comm_init")

    def comm_info(self):
        """(world, rank) of the handle's communicator as RCCL reports them (ncclCommCount,
        ncclCommUserRank)"""
        w, r = C.c_int(), C.c_int()
        check(load().fmskf_comm_info(self.h, C.byref(w), C.byref(r)), "comm_info")
        return w.value, r.value

    def ensemble_stats(self):
        """(mean [n], cov packed [n(n+1)/2]) over all ranks of the communicator (or this
        handle alone): device record, ncclAllGather, rank-order fold"""
        nx = self.nx
        mean = np.empty(nx, np.float64)
        cov = np.empty(nx * (nx + 1) // 2, np.float64)
        check(load().fmskf_ensemble_stats(self.h, mean.ctypes.data_as(C.c_void_p),
                                          cov.ctypes.data_as(C.c_void_p)), "ensemble_stats")
        return mean, cov

    def tick_ensemble_begin(self, prepared=None, **kw):
        """fmskf_tick_ensemble_begin: one tick whose kernel also writes this rank's ensemble
        record; fold + all-gather + copy-out run on the handle's side stream (no host wait).
        `prepared` (from prepare()) or tick inputs as keywords."""
        if prepared is not None:
            ref = prepared[2]
        else:
            ti, _keep = self._inputs(kw)
            ref = C.byref(ti)
        check(load().fmskf_tick_ensemble_begin(self.h, ref), "tick_ensemble_begin")

    def ensemble_begin(self):
        """fmskf_ensemble_begin: the stand-alone record of the current state, asynchronously"""
        check(load().fmskf_ensemble_begin(self.h), "ensemble_begin")

    def ensemble_end(self):
        """fmskf_ensemble_end: (mean, cov packed) of the oldest pending begin"""
        nx = self.nx
        mean = np.empty(nx, np.float64)
        cov = np.empty(nx * (nx + 1) // 2, np.float64)
        check(load().fmskf_ensemble_end(self.h, mean.ctypes.data_as(C.c_void_p),
                                        cov.ctypes.data_as(C.c_void_p)), "ensemble_end")
        return mean, cov

    def ensemble_end_count(self):
        """fmskf_ensemble_end_count: (mean, cov packed, robots the gathered records count,
        records folded) of the oldest pending begin"""
        nx = self.nx
        mean = np.empty(nx, np.float64)
        cov = np.empty(nx * (nx + 1) // 2, np.float64)
        cnt, nrec = C.c_double(), C.c_uint32()
        check(load().fmskf_ensemble_end_count(self.h, mean.ctypes.data_as(C.c_void_p),
                                              cov.ctypes.data_as(C.c_void_p), C.byref(cnt), C.byref(nrec)),
              "ensemble_end_count")
        return mean, cov, cnt.value, nrec.value

    def ensemble_exchange_ms(self) -> float:
        """fmskf_ensemble_exchange_ms: the side stream's all-gather + copy-out time of the result
        the last ensemble_end collected (ms), -1 when it needed no exchange"""
        ms = C.c_float()
        check(load().fmskf_ensemble_exchange_ms(self.h, C.byref(ms)), "ensemble_exchange_ms")
        return ms.value

    # ------------------------------------------------------------------ control step
    def set_ctrl_params(self, **kw):
        """FF_PI_D / interpolator / current-limit parameters (fmskf_ctrl_params); unspecified
        fields keep the firmware defaults (VD_task_main.cpp:86-97,157-160)."""
        p = CtrlParams()
        check(load().fmskf_ctrl_params_init(C.byref(p)), "ctrl_params_init")
        for k, v in kw.items():
            setattr(p, k, v)
        check(load().fmskf_set_ctrl_params(self.h, C.byref(p)), "set_ctrl_params")

    def set_power(self, on=None):
        """on: None (all on), a scalar or [N] host array, or an [N] uint8 device tensor (a call
        that is captured)"""
        a = _Args()
        if on is not None and _is_torch(on) and on.is_cuda:
            if str(on.dtype) != "torch.uint8" or on.numel() < self.n:
                raise TypeError(f"on: want an [N] uint8 device tensor, got {on.dtype} x {on.numel()}")
            p = a.ptr(on)
        else:
            p = a.ptr(None if on is None else np.broadcast_to(np.asarray(on, np.uint8), (self.n,)),
                      np.uint8)
        check(load().fmskf_set_power(self.h, p, MEM_HOST if a.mem is None else a.mem), "set_power")

    def set_target_vel(self, vel, acl, jrk, mask=None):
        """vel/acl/jrk [3][N] (x mm/s, y mm/s, th rad/s)"""
        a = _Args()
        ps = [a.ptr(v, np.float32) for v in (vel, acl, jrk)]
        for name, v in zip(("vel", "acl", "jrk"), (vel, acl, jrk)):
            have = v.numel() if _is_torch(v) else np.size(v)
            if have < 3 * self.n:
                raise ValueError(f"{name}: {have} elements, need 3*N = {3 * self.n}")
        pm = a.ptr(mask, np.uint8)
        check(load().fmskf_set_target_vel(self.h, *ps, pm, MEM_HOST if a.mem is None else a.mem),
              "set_target_vel")

    def control(self, rpm=None):
        a = _Args()
        if rpm is not None:
            have = rpm.numel() if _is_torch(rpm) else np.size(rpm)
            if have < 4 * self.n:
                raise ValueError(f"rpm: {have} elements, need 4*N = {4 * self.n}")
        p = a.ptr(rpm, np.int16)
        check(load().fmskf_control(self.h, p, MEM_HOST if a.mem is None else a.mem), "control")

    def can_tx(self, out=None):
        """CAN_CTRL::tx_routine payloads [N][8] (host numpy, or into a device tensor `out`)"""
        if out is not None and _is_torch(out) and out.is_cuda:
            check(load().fmskf_can_tx(self.h, C.c_void_p(out.data_ptr()), MEM_DEVICE), "can_tx")
            return out
        f = np.empty((self.n, 8), np.uint8)
        check(load().fmskf_can_tx(self.h, f.ctypes.data_as(C.c_void_p), MEM_HOST), "can_tx")
        return f

    def isr_tick(self, frames=True, out=None, **kw):
        """VDT::can_tx_routine_intr in one call (fmskf_isr_tick): correct, update (estimator +
        control), tx_routine.  Inputs as tick(); returns the [N][8] frames (host numpy, or the
        device tensor `out`), or None with frames=False."""
        ti, _keep = self._inputs(kw)
        if out is not None and _is_torch(out) and out.is_cuda:
            check(load().fmskf_isr_tick(self.h, C.byref(ti), C.c_void_p(out.data_ptr()), MEM_DEVICE),
                  "isr_tick")
            return out
        if not frames:
            check(load().fmskf_isr_tick(self.h, C.byref(ti), None, MEM_HOST), "isr_tick")
            return None
        f = np.empty((self.n, 8), np.uint8)
        check(load().fmskf_isr_tick(self.h, C.byref(ti), f.ctypes.data_as(C.c_void_p), MEM_HOST),
              "isr_tick")
        return f

    def isr_tick_can(self, can_frames, can_stamps, frames=True, out=None, **kw):
        """The tick's CAN RX and the ISR in one call (fmskf_isr_tick_can): ingest_can(can_frames,
        can_stamps) then isr_tick(**kw), one kernel for RS, KF6 and EKF9.  can_frames [N, 4, 8] uint8,
        can_stamps [N, 4] int16, both host arrays or both device tensors; the [N][8] TX frames
        come back the same way (numpy, or the device tensor `out`), None with frames=False."""
        a = _Args()
        pf = a.ptr(can_frames, np.uint8)
        ps = a.ptr(can_stamps, np.int16)
        for name, v, per in (("can_frames", can_frames, 32), ("can_stamps", can_stamps, 4)):
            have = v.numel() if _is_torch(v) else np.size(v)
            if have < per * self.n:
                raise ValueError(f"{name}: {have} elements, need {per}*N = {per * self.n}")
        mem = MEM_HOST if a.mem is None else a.mem
        ti, _keep = self._inputs(kw)
        if not frames:
            check(load().fmskf_isr_tick_can(self.h, pf, ps, C.byref(ti), None, mem), "isr_tick_can")
            return None
        if mem == MEM_DEVICE:
            import torch
            if out is None:
                out = torch.empty((self.n, 8), dtype=torch.uint8, device=can_frames.device)
            if not (_is_torch(out) and out.is_cuda):
                raise TypeError("device CAN frames need a device `out`")
            check(load().fmskf_isr_tick_can(self.h, pf, ps, C.byref(ti), C.c_void_p(out.data_ptr()), mem),
                  "isr_tick_can")
            return out
        if out is not None:  # one mem flag covers the CAN buffers and the TX frames
            raise TypeError("host CAN frames: the TX frames come back as a numpy array (out=None)")
        f = np.empty((self.n, 8), np.uint8)
        check(load().fmskf_isr_tick_can(self.h, pf, ps, C.byref(ti), f.ctypes.data_as(C.c_void_p), mem),
              "isr_tick_can")
        return f

    def get_ctrl(self):
        vt = np.empty((3, self.n), np.float32)
        cur = np.empty((self.n, 4), np.int16)
        wt = np.empty((4, self.n), np.float32)
        wc = np.empty((4, self.n), np.float32)
        check(load().fmskf_get_ctrl(self.h, *(x.ctypes.data_as(C.c_void_p) for x in (vt, cur, wt, wc)),
                                    MEM_HOST), "get_ctrl")
        return dict(vel_tgt=vt, curr=cur, wheel_tgt=wt, wheel_ctrl=wc)

    def export_vehicle_info(self, floor=None, cam_pitch=None, fault=None, out=None):
        """[N] VehicleInfo records: a structured numpy array (VEHICLE_INFO_DTYPE) from host
        inputs; with `out`, an [N, 84] uint8 device tensor, the records' bytes on the device (one
        mem flag covers the call: floor [N, 8] uint8, cam_pitch [N] float32 and fault [N] must
        then be device tensors too, or None).  Device inputs without `out` get a new tensor."""
        a = _Args()
        dev = None
        # the C ABI takes bare pointers: check the device tensors' types and extents here
        # (fault: any 32-bit integer type, torch builds differ in their uint32 support)
        for name, v, dt, cnt in (("floor", floor, "uint8", 8 * self.n), ("cam_pitch", cam_pitch, "float32", self.n),
                                 ("fault", fault, None, self.n)):
            if v is not None and _is_torch(v) and v.is_cuda:
                dev = v.device
                ok = (v.element_size() == 4 and not v.is_floating_point()) if dt is None \
                    else str(v.dtype) == "torch." + dt
                if not ok or v.numel() < cnt:
                    raise TypeError(f"{name}: dtype {v.dtype} x {v.numel()}, want {dt or 'int32'} x {cnt}")
        pf = a.ptr(floor, np.uint8)
        pc = a.ptr(cam_pitch, np.float32)
        pu = a.ptr(fault, np.uint32)
        if out is not None or a.mem == MEM_DEVICE:
            if out is None:
                import torch
                out = torch.empty((self.n, VEHICLE_INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            if not (_is_torch(out) and out.is_cuda and str(out.dtype) == "torch.uint8"
                    and out.numel() == self.n * VEHICLE_INFO_DTYPE.itemsize):
                raise TypeError("export_vehicle_info: `out` must be an [N, 84] uint8 device tensor")
            po = a.ptr(out)  # raises when the inputs are host arrays
            check(load().fmskf_export_vehicle_info(self.h, po, pf, pc, pu, MEM_DEVICE), "export_vehicle_info")
            return out
        out = np.empty(self.n, VEHICLE_INFO_DTYPE)
        check(load().fmskf_export_vehicle_info(self.h, out.ctypes.data_as(C.c_void_p), pf, pc, pu,
                                               MEM_HOST), "export_vehicle_info")
        return out

    def get_counters(self):
        out = (C.c_uint64 * 8)()
        check(load().fmskf_get_counters(self.h, out, 8), "get_counters")
        return list(out)

    # ------------------------------------------------------------------ ensemble
    def ensemble_record_len(self) -> int:
        v = C.c_uint32()
        check(load().fmskf_ensemble_record_len(self.h, C.byref(v)), "ensemble_record_len")
        return v.value

    def ensemble_partial(self, out=None):
        """This rank's {count, mean, M2} record: numpy (host) or into a torch CUDA tensor."""
        if out is not None and _is_torch(out) and out.is_cuda:
            check(load().fmskf_ensemble_partial(self.h, C.c_void_p(out.data_ptr()), MEM_DEVICE),
                  "ensemble_partial")
            return out
        rec = np.empty(self.ensemble_record_len(), np.float64)
        check(load().fmskf_ensemble_partial(self.h, rec.ctypes.data_as(C.c_void_p), MEM_HOST),
              "ensemble_partial")
        return rec

    def tick_ensemble(self, out=None, **kw):
        """fmskf_tick_ensemble: one tick plus this rank's record of the post-tick state"""
        ti, _keep = self._inputs(kw)
        return self._tick_ens(C.byref(ti), out)

    def tick_ensemble_prepared(self, prepared, out=None):
        return self._tick_ens(prepared[2], out)

    def _tick_ens(self, ti_ref, out):
        if out is not None and _is_torch(out) and out.is_cuda:
            check(load().fmskf_tick_ensemble(self.h, ti_ref, C.c_void_p(out.data_ptr()), MEM_DEVICE),
                  "tick_ensemble")
            return out
        rec = np.empty(self.ensemble_record_len(), np.float64)
        check(load().fmskf_tick_ensemble(self.h, ti_ref, rec.ctypes.data_as(C.c_void_p), MEM_HOST),
              "tick_ensemble")
        return rec

    # ------------------------------------------------------------------ diagnostics
    def eval_trig(self, x):
        x = np.ascontiguousarray(x, np.float32)
        s = np.empty_like(x)
        c = np.empty_like(x)
        check(load().fmskf_eval_trig(self.h, x.ctypes.data_as(C.c_void_p),
                                     s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                     x.size, MEM_HOST), "eval_trig")
        return s, c


def ensemble_combine(n_state: int, records) -> tuple[np.ndarray, np.ndarray]:
    """Fold per-rank records in rank order -> (mean [n], covariance packed [n(n+1)/2])."""
    recs = np.ascontiguousarray(records, np.float64)
    nrec = recs.shape[0] if recs.ndim == 2 else 1
    mean = np.empty(n_state, np.float64)
    cov = np.empty(n_state * (n_state + 1) // 2, np.float64)
    check(load().fmskf_ensemble_combine(n_state, recs.ctypes.data_as(C.c_void_p), nrec,
                                        mean.ctypes.data_as(C.c_void_p),
                                        cov.ctypes.data_as(C.c_void_p)), "ensemble_combine")
    return mean, cov


def loglik(nis_sum, logdet_sum, n_meas):
    """The innovation log-likelihood of Engine.tick_many_loglik's sums (per robot, or of the fleet's
    total[1], total[2], total[0]): -0.5 * (nis + logdet + 4 * n * log(2 pi)).  numpy or torch."""
    return -0.5 * (nis_sum + logdet_sum + 4.0 * n_meas * float(np.log(2.0 * np.pi)))


def em_mstep(total):
    """fmskf_em_mstep: the M-step of Engine.tick_many_em's fleet total [34] (a numpy array, or a
    torch tensor, which is copied to the host): (q [21], r [10]), the packed Q and R a new
    Engine(q=, r=) takes.  FMSKF_EINVAL for a total without transitions or measurements or with a
    non-finite entry."""
    if total is None:
        tp = None
    else:
        t = np.ascontiguousarray(total.cpu().numpy() if _is_torch(total) else total, np.float64)
        if t.shape != (_lib.EM_TOTAL_LEN,):
            raise ValueError(f"em_mstep: total has shape {t.shape}, want {(_lib.EM_TOTAL_LEN,)}")
        tp = t.ctypes.data
    q, r = np.empty(21, np.float64), np.empty(10, np.float64)
    check(load().fmskf_em_mstep(tp, q.ctypes.data, r.ctypes.data), "em_mstep")
    return q, r


def shard_span(n_total: int, world: int, rank: int) -> tuple[int, int]:
    """Rank `rank`'s contiguous robot range [lo, hi) of `n_total` over `world` ranks, the
    remainder on the first ranks (bench.py's sharding): shards differ by at
    most one robot and rank order is robot order, so the rank-order fold of the records is
    the fold of the unsharded fleet."""
    if world < 1 or not 0 <= rank < world or n_total < 0:
        raise ValueError(f"shard_span: n_total {n_total}, world {world}, rank {rank}")
    base, rem = divmod(n_total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def rccl_library() -> str:
    """the file libfmskf resolved RCCL from ("" before its first communicator call)"""
    v = load().fmskf_rccl_library()
    return v.decode() if v else ""


def comm_unique_id() -> bytes:
    """fmskf_comm_unique_id (rank 0): 128 bytes to hand to every rank's comm_init"""
    b = (C.c_uint8 * 128)()
    check(load().fmskf_comm_unique_id(b), "comm_unique_id")
    return bytes(b)


def default_config(model="kf6", n=1) -> Config:
    """Model defaults (pure host call, no GPU needed)."""
    cfg = Config()
    m = MODEL_NAMES[model] if isinstance(model, str) else int(model)
    check(load().fmskf_config_init(C.byref(cfg), m, int(n)), "config_init")
    return cfg


__all__ = ["Engine", "pose_fix_records", "POSE_FIX_DTYPE", "range_fix_records", "RANGE_FIX_DTYPE", "ensemble_combine", "default_config", "comm_unique_id", "VEHICLE_INFO_DTYPE", "MODEL_RS", "MODEL_KF6", "MODEL_EKF9",
           "MODEL_KF12D", "TRIG_TABLE512", "TRIG_LIBM", "_lib"]
