from spline_trajectory_optimization_amd.utils.integrator import hermite_simpson, rk4  # noqa: F401
