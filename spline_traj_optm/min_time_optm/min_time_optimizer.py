from spline_trajectory_optimization_amd.min_time_optm.min_time_optimizer import (  # noqa: F401
    BicycleProblem, DoubleTrackProblem, fold_margins, optimise_track, optimise_track_batch, optimise_tracks_batch, set_up_bicycle_problem,
    set_up_double_track_problem, vehicle_margins)
