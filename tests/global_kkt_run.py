"""One case of tests/global_kkt_cases.py solved on the kernels in a process of its own, for the switches that the library reads
when its context is created (RL_GLOBAL_V1=1: the generic kernel on n_p <= 64).  usage: global_kkt_run.py OUT.npz CASE_ID
Writes x, st (the m-run), xp, stp (the hooked (m-1)-run) and the block size of the last launch."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import global_kkt_cases as gk  # noqa: E402

out, tag = sys.argv[1], sys.argv[2]
solver = gk.KernelSolver()
x, st, xp, stp = gk.solve_case(solver, gk.by_id(tag))
np.savez(out, x=x, st=st, xp=xp, stp=stp, block_threads=solver.last_rs.block_threads)
