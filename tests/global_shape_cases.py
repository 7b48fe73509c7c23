"""Synthetic closed splines for the one-offset global min-curvature QP, and a restatement of its kernel dispatch.

THE FAMILY.  A closed periodic B-spline built directly (no FITPACK): breakpoints 0 = b_0 < ... < b_np = 1, extended
periodically by k knots on each side (nt = n_p + 2k + 1 knots, n = n_p + k control points, the last k equal to the first k:
the splprep(per=True) convention of the library).  Control points lie on r(theta) = 100 (1 + 0.25 cos 2 theta + 0.1 sin 3 theta)
m at the Greville abscissae; half-widths w_l = 5 + sin(0.02 i), w_r = 4.5 + cos(0.03 i); margin 0.25 m.  Breakpoints are
uniform, or "uneven": seeded, two spans 1e-3 of the mean width and one span six times it -- at N close to 2 n_p that leaves
spans without a sample (no chunk at all) and tail chunks shorter than R.

THE MIRROR.  dispatch(t, k, N, max_lds) restates global_tables / global_common of csrc/rl_mincurv.hip: rows per knot span,
chunk counts for R = 5, 6, 10 (fast path) and 8 (generic kernel), the lane-group count, both LDS layouts (global2_layout of
rl_global2.hpp, global_layout of rl_global.hpp) and the fall-backs.  The GPU test compares its block_threads / lds_bytes with
the rl_stats of the call; a test names a branch only while that comparison holds.

THE CASE LIST is fixed.  Every case names the branch it is there for (`expect`, at 160 KiB of LDS);
tests/test_global_shapes_cpu.py holds the mirror to it case by case and the set of branches reached to BRANCHES_160K, so a
dropped case cannot silently drop a branch.  Choices of this file where the shape was free: n_p = 4k runs at N = 201 (at
N = 200, K = 5 the twin's own strict-versus-FMA spread is 3.4e-9 m, above the 1e-9 m the GPU bound presumes)."""
from dataclasses import dataclass

import numpy as np

MARGIN = 0.25
LDS_160K = 160 * 1024

# csrc/rl_global.hpp, rl_global2.hpp
G_ROWS, G_ROUND, G_MAX_NP, G2_BLOCK = 8, 11, 192, 512


# ------------------------------------------------------------------------------------------------------- the family
def breakpoints(n_p, uneven_seed=None):
    if uneven_seed is None:
        return np.arange(n_p + 1) / float(n_p)
    rng = np.random.default_rng(uneven_seed)
    w = rng.uniform(0.8, 1.2, n_p)
    thin0, thin1, fat = rng.choice(n_p, 3, replace=False)
    if uneven_seed % 2 == 0:                  # two empty spans in a row
        thin1 = (thin0 + 1) % n_p
        fat = (thin0 + n_p // 2) % n_p
    mean = w.mean()
    w[thin0] = w[thin1] = 1e-3 * mean
    w[fat] = 6.0 * mean
    b = np.r_[0.0, np.cumsum(w)]
    b /= b[-1]
    b[-1] = 1.0
    return b


def closed_spline(k, n_p, uneven_seed=None):
    """-> (t [n_p + 2k + 1], cx [n_p + k], cy [n_p + k])."""
    b = breakpoints(n_p, uneven_seed)
    t = np.r_[b[n_p - k:n_p] - 1.0, b, b[1:k + 1] + 1.0]
    assert len(t) == n_p + 2 * k + 1 and (np.diff(t) > 0).all()
    g = np.array([t[j + 1:j + k + 1].mean() for j in range(n_p)])
    th = 2.0 * np.pi * g
    r = 100.0 * (1.0 + 0.25 * np.cos(2.0 * th) + 0.1 * np.sin(3.0 * th))
    cx, cy = r * np.cos(th), r * np.sin(th)
    return t, np.r_[cx, cx[:k]], np.r_[cy, cy[:k]]


def half_widths(N, scale=1.0):
    i = np.arange(N)
    return scale * (5.0 + np.sin(0.02 * i)), scale * (4.5 + np.cos(0.03 * i))


def weights_sine(N):
    return 1.0 + 0.5 * np.sin(0.05 * np.arange(N))


# -------------------------------------------------------------------------------------------------------- the mirror
def rows_per_span(t, k, N):
    """Samples u_i = i (1/N) per knot span: host_find_interval of global_tables (the largest l in [k, n-1] with t[l] <= u)."""
    n = len(t) - k - 1
    u = np.arange(N, dtype=np.float64) * (1.0 / N)
    ell = np.clip(np.searchsorted(t[:n], u, side="right") - 1, k, n - 1)
    return np.bincount(ell - k, minlength=n - k)


def n_chunks(rows, R):
    return int(((rows + R - 1) // R).sum())


def _even(c):
    return (c + 1) & ~1


def global2_layout_doubles(k, n, n_p, N, groups, nrow):
    K1, NS = k + 1, 4 * k + 1
    NO = K1 * (K1 + 1) // 2 + 2 * K1
    rnd = 17 if groups == 1 else 12
    mf = NS * 64 + NS * 32 + 128 if groups == 1 else NS * 64 * groups
    parts = [n_p] * 9 + [n, n, 2 * n_p, n_p * K1, n_p * K1, (NS * 64 + NS * 32 + 3) // 4 if groups == 1 else 0, n_p * NO,
             max(nrow * rnd, mf), 2 * N, 4 * 16, 8, (n_p + 2) // 2 + 1]
    return sum(_even(c) for c in parts)


def global_layout_doubles(k, n, n_p, block):
    K1 = k + 1
    NO = K1 * (K1 + 1) // 2 + 2 * K1
    return 8 * n_p + 2 * n + 2 * n_p + 2 * n_p * K1 + k * n_p + n_p * NO + block * G_ROUND + 3 * 16 + (n_p + 2) // 2 + 1


@dataclass(frozen=True)
class Dispatch:
    family: str            # "qp2" | "qp" | "refused"
    R: int                 # rows per thread
    G: int                 # lane groups of the factorisation (qp2), else 0
    template: int          # block-size template of k_global_qp, else 0
    block_threads: int
    lds_bytes: int
    why: str               # qp: why not the fast path ("forced" | "chunks" | "r10_g3" | "lds"); refused: the library's message
    empty_spans: int
    short_tails: int       # chunks of the chosen partition with fewer than R rows
    n_chunks: int

    @property
    def branch(self):
        if self.family == "qp2":
            return f"qp2 R{self.R}G{self.G}"
        if self.family == "qp":
            return f"qp <{self.template}> {self.why}"
        return f"refused: {self.why}"


def dispatch(t, k, N, max_lds=LDS_160K, force_v1=False):
    n = len(t) - k - 1
    n_p = n - k
    rows = rows_per_span(t, k, N)
    empty = int((rows == 0).sum())

    def refused(msg):
        return Dispatch("refused", 0, 0, 0, 0, 0, msg, empty, 0, 0)

    if n_p < 2 * (k + 1):
        return refused("too few control points")
    if n_p > G_MAX_NP:
        return refused("more than 192 free control points")
    nc8 = n_chunks(rows, G_ROWS)
    R2, nc2 = 0, 0
    for R in (5, 6, 10):
        nc2 = n_chunks(rows, R)
        if nc2 <= G2_BLOCK - 64:
            R2 = R
            break
    if nc8 > 1024:
        return refused("N / 8 + n exceeds one workgroup")
    why = "forced" if force_v1 else "chunks"
    if not force_v1 and R2 != 0:
        groups = 1 if n_p <= 64 else 3
        block2 = ((nc2 + 63) // 64 + 1) * 64
        lds2 = 8 * global2_layout_doubles(k, n, n_p, N, groups, block2 - 64)
        if lds2 > max_lds:
            why = "lds"
        elif R2 == 10 and groups != 1:
            why = "r10_g3"
        else:
            short = int(((rows % R2) != 0).sum())
            return Dispatch("qp2", R2, groups, 0, block2, lds2, "", empty, short, nc2)
    block = max(64, (nc8 + 63) // 64 * 64)
    lds = 8 * global_layout_doubles(k, n, n_p, block)
    if lds > max_lds:
        return refused("does not fit LDS")
    template = 384 if block <= 384 else (640 if block <= 640 else 1024)
    return Dispatch("qp", G_ROWS, 0, template, block, lds, why, empty, int(((rows % G_ROWS) != 0).sum()), nc8)


# --------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    k: int
    n_p: int
    N: int
    expect: str            # Dispatch.branch at 160 KiB
    n_outer: int = 3
    uneven_seed: int = None
    force_v1: bool = False    # run on a context created under RL_GLOBAL_V1=1

    @property
    def id(self):
        return f"k{self.k}-{self.name}"

    @property
    def problem(self):
        """What the twin sees: cases that differ in the context alone share it."""
        return (self.k, self.n_p, self.N, self.n_outer, self.uneven_seed)

    def spline(self):
        return closed_spline(self.k, self.n_p, self.uneven_seed)

    def dispatch(self, max_lds=LDS_160K):
        return dispatch(self.spline()[0], self.k, self.N, max_lds, self.force_v1)


TOO_MANY = "refused: more than 192 free control points"


def _cases_of(k):
    C = []

    def add(name, n_p, N, expect, **kw):
        C.append(Case(name, k, n_p, N, expect, **kw))

    # fast path, one lane group (TwoFront<2k>::fronts(n_p) = (n_p - 4k) / 2 front columns): none up to n_p = 4k + 1, where the
    # middle block is full (4k + 1 rows), and the first one at n_p = 4k + 2
    add("np_min_N100", 2 * (k + 1), 100, "qp2 R5G1")
    add("np_4k_N201", 4 * k, 201, "qp2 R5G1")
    add("np_4k_N201_outer1", 4 * k, 201, "qp2 R5G1", n_outer=1)
    add("np_4k1_N333", 4 * k + 1, 333, "qp2 R5G1")
    add("np_4k1_N333_outer1", 4 * k + 1, 333, "qp2 R5G1", n_outer=1)
    add("np_4k2_N333", 4 * k + 2, 333, "qp2 R5G1")
    add("np_4k2_N333_outer1", 4 * k + 2, 333, "qp2 R5G1", n_outer=1)
    add("np27_N257", 27, 257, "qp2 R5G1")
    add("np27_N257_outer1", 27, 257, "qp2 R5G1", n_outer=1)
    add("np63_N500", 63, 500, "qp2 R5G1")
    add("np64_N500", 64, 500, "qp2 R5G1")
    add("np64_N500_outer1", 64, 500, "qp2 R5G1", n_outer=1)
    add("np64_N500_outer6", 64, 500, "qp2 R5G1", n_outer=6)
    add("np64_N2239", 64, 2239, "qp2 R5G1")        # 448 chunks: the last R = 5
    add("np64_N2241", 64, 2241, "qp2 R6G1")        # 449 chunks of 5
    add("np64_N2700", 64, 2700, "qp2 R10G1")
    # fast path, three lane groups (FoldBand)
    add("np65_N131", 65, 131, "qp2 R5G3")
    add("np65_N500", 65, 500, "qp2 R5G3")
    add("np65_N500_outer1", 65, 500, "qp2 R5G3", n_outer=1)
    add("np66_N999", 66, 999, "qp2 R5G3")
    add("np66_N999_outer1", 66, 999, "qp2 R5G3", n_outer=1)
    add("np128_N1000", 128, 1000, "qp2 R5G3")      # rows on both sides of a lane-group boundary
    add("np129_N1000", 129, 1000, "qp2 R5G3")
    add("np191_N2001", 191, 2001, "qp2 R6G3")
    add("np192_N2000", 192, 2000, "qp2 R6G3")
    # generic kernel, not forced
    add("np100_N3000", 100, 3000, "qp <640> r10_g3")
    add("np100_N3000_outer6", 100, 3000, "qp <640> r10_g3", n_outer=6)
    add("np48_N5600", 48, 5600, "qp <1024> chunks")
    add("np192_N2303", 192, 2303, "qp2 R6G3" if k == 3 else "qp <384> lds")     # K = 5: the fast layout is 164256 B
    add("np192_N3000", 192, 3000, "qp <384> r10_g3" if k == 3 else "qp <384> lds")
    add("np192_N3500", 192, 3500, "qp <640> r10_g3" if k == 3 else "qp <640> lds")
    # <1024> at the largest n_p.  K = 5: N = 5000 needs 768 threads, whose generic layout is 164064 B > 160 KiB and is refused;
    # N = 4736 is the largest N the layout accepts on that template (704 threads, 158432 B)
    add("np192_N5000", 192, 5000, "qp <1024> chunks" if k == 3 else "refused: does not fit LDS")
    if k == 5:
        add("np192_N4736", 192, 4736, "qp <1024> chunks")
    # past the largest n_p: global_tables refuses (the triangular solves of both kernels hold three rows per lane), so the
    # generic kernel is never reached by n_p > 192; the three templates are pinned by the n_p <= 192 cases above
    add("np193_N579", 193, 579, TOO_MANY)
    add("np193_N2000", 193, 2000, TOO_MANY)
    add("np200_N5000", 200, 5000, TOO_MANY)
    # uneven breakpoints: empty spans and short tail chunks, on the fast path and on the generic kernel
    for n_p, N, seed in ((40, 97, 11), (64, 131, 12), (90, 181, 13)):
        add(f"uneven_np{n_p}_N{N}", n_p, N, "qp2 R5G1" if n_p <= 64 else "qp2 R5G3", uneven_seed=seed)
        add(f"uneven_np{n_p}_N{N}_v1", n_p, N, "qp <384> forced", uneven_seed=seed, force_v1=True)
    return C


CASES = _cases_of(3) + _cases_of(5)
BY_ID = {c.id: c for c in CASES}
RUNNABLE = [c for c in CASES if not c.expect.startswith("refused")]

# every (degree, branch) the dispatch has: five fast instantiations and three generic templates per degree, the generic ones by
# every reason that leads there (three groups would need R = 10; chunks beyond seven row waves; LDS overflow of the fast
# layout, which needs K = 5; forced), and the two refusals
BRANCHES_160K = {(k, b) for k in (3, 5) for b in (
    "qp2 R5G1", "qp2 R6G1", "qp2 R10G1", "qp2 R5G3", "qp2 R6G3",
    "qp <384> forced", "qp <640> r10_g3", "qp <1024> chunks", TOO_MANY)} | {
    (3, "qp <384> r10_g3"),
    (5, "qp <384> lds"), (5, "qp <640> lds"), (5, "refused: does not fit LDS")}

# one case per (family, R, G | template) and degree for the weighted cost against tests/weighted_global_twin.py
WEIGHTED_VS_TWIN = [f"k{k}-{name}" for k in (3, 5) for name in (
    "np64_N500", "np64_N2241", "np64_N2700", "np129_N1000", "np191_N2001", "np192_N3000", "np100_N3000", "np48_N5600",
    "uneven_np64_N131", "uneven_np64_N131_v1")]

# n_outer = 1, n_p <= 66: certified on the dense numpy statement of the QP (tests/test_global_qp.py: NumpyGlobal)
CERTIFIED = [c.id for c in CASES if c.n_outer == 1]
