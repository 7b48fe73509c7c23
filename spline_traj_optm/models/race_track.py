from spline_trajectory_optimization_amd.models.race_track import RaceTrack, interval_for_nodes, race_track_with_nodes  # noqa: F401
