"""fmskf -- MI355X-native batched IMU + mecanum-odometry state estimation.

Host-side mirror of the C ABI in include/fmskf.h (libfmskf.so, HIP kernels for
gfx950).  See DESIGN.md for the hot path, its boundary and the data layout.
"""
from ._lib import (ABI_VERSION, CFG_COMP_POS, FIX_HEADING, FIX_IGNORED, GATE_ACCEPTED, GATE_FORCED, GATE_NONE, GATE_REJECTED, EM_ACCUMULATE, LL_ACCUMULATE, MEM_DEVICE, MEM_HOST, MODEL_EKF9, MODEL_KF6, MODEL_KF12D,
                   MODEL_RS, RANGE_ANCHORS_MAX, RANGE_NEAR, RANGE_RUN_MAX, ROW_GATE_D2, SEL_GATE_RUN, SEL_NONFINITE, SEL_POS_VAR, TRIG_LIBM, TRIG_TABLE512, EKF9_ROWS, FmskfError, load)
from .engine import (KF6_RECORD_DTYPE, POSE_FIX_DTYPE, RANGE_FIX_DTYPE, Engine, comm_unique_id, default_config, em_mstep, ensemble_combine,
                     kf6_records, loglik, pose_fix_records, range_fix_records, rccl_library, shard_span)

__all__ = ["Engine", "default_config", "ensemble_combine", "FmskfError", "load", "ABI_VERSION",
           "MEM_HOST", "MEM_DEVICE", "MODEL_RS", "MODEL_KF6", "MODEL_EKF9", "MODEL_KF12D",
           "TRIG_TABLE512", "TRIG_LIBM", "KF6_RECORD_DTYPE", "kf6_records", "shard_span",
           "CFG_COMP_POS", "rccl_library", "GATE_NONE", "GATE_ACCEPTED", "GATE_REJECTED", "GATE_FORCED",
           "FIX_HEADING", "FIX_IGNORED", "POSE_FIX_DTYPE", "pose_fix_records",
           "RANGE_FIX_DTYPE", "range_fix_records", "RANGE_NEAR", "RANGE_RUN_MAX", "RANGE_ANCHORS_MAX",
           "EKF9_ROWS", "ROW_GATE_D2", "SEL_NONFINITE", "SEL_POS_VAR", "SEL_GATE_RUN", "LL_ACCUMULATE", "loglik",
           "EM_ACCUMULATE", "em_mstep"]
