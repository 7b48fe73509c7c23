"""The reference's console tools (its setup.py `console_scripts`): traj_opt_double_track, traj_opt_encode_region and
traj_opt_convert_to_casadi.  Each module has a `main()` and runs with `python -m`."""
