"""The reference's console tools under its module paths (spline_traj_optm.entrypoints.*), re-exported."""
