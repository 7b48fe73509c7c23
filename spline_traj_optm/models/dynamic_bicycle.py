from spline_trajectory_optimization_amd.models.dynamic_bicycle import (  # noqa: F401
    dynamics, lat_acc, lon_acc, nu, nx, u_l, u_u, x_l, x_u)
