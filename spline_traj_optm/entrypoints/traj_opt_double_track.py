from spline_trajectory_optimization_amd.entrypoints.traj_opt_double_track import main  # noqa: F401

if __name__ == "__main__":
    main()
