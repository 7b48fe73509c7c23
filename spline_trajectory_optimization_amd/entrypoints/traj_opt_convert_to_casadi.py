"""traj_opt_convert_to_casadi <TTL_in> <txt_out>: a TTL file as a CasADi "txt" matrix of its columns X .. TIME, with SPEED
set to -100 (entrypoints/traj_opt_convert_to_casadi.py of the reference)."""
import sys

from ..models.trajectory import Trajectory, load_ttl
from ..utils.casadi_txt import write_txt

USAGE = "Usage: python3 -m spline_trajectory_optimization_amd.entrypoints.traj_opt_convert_to_casadi <TTL_in> <casadi_txt_out>"


def main(argv=None):
    args = sys.argv[1:] if argv is None else list(argv)
    if len(args) != 2:
        print(USAGE)
        return
    ttl_in, txt_out = args
    ttl = load_ttl(ttl_in)
    ttl[:, Trajectory.SPEED] = -100.0
    write_txt(txt_out, ttl.points[:, :Trajectory.TIME + 1])


if __name__ == "__main__":
    main()
