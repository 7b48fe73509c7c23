from spline_trajectory_optimization_amd.utils.utils import align_abscissa, align_yaw, global_to_frenet  # noqa: F401
