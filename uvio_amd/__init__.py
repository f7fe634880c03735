"""uvio_amd — MI355X-native implementation of the uvio/OpenVINS per-frame hot path
(track -> propagate -> MSCKF/SLAM/UWB update -> EKF update) behind a C ABI (include/uvio_hp.h).

The estimator runs in ``libuvio_hp.so`` (host C++ orchestration + gfx950 HIP kernels).  This package
only binds it: ``VioManager`` mirrors ov_msckf::VioManager / uvio::UVioManager.
"""
from . import _native  # noqa: F401
from .manager import (VioManager, apply_overrides, aux_append_p, aux_init_p, aux_walk_p, chi2_95, clahe,  # noqa: F401
                      compress, cov_gather_p, cov_propagate_p, draw_tracks, ekf_update, ekf_update_R, load_options, loop_depth,
                      position_fix_jacobian, position_fix_lever_arm_jacobian, pose_update_p, position_update_p,
                      undistort)

__all__ = ["VioManager", "load_options", "apply_overrides", "ekf_update", "compress", "undistort", "clahe",
           "draw_tracks", "loop_depth", "ekf_update_R", "chi2_95", "position_fix_jacobian",
           "position_fix_lever_arm_jacobian", "aux_append_p", "aux_init_p", "aux_walk_p",
           "position_update_p", "pose_update_p", "cov_propagate_p", "cov_gather_p"]
