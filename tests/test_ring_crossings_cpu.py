"""The CPU oracle's fill_bounds (oracle/mincurv_oracle.c: closest_hit) against the exact reference of tests/ring_cases.py, on
exact ties, vertex hits, collinear edges, the range limit, zero distance, combs, underflowing side values and rings without a
hit -- in the strict build, the FMA-contracted build and the build with the correctly rounded cos / sin.  Every asserted
bound column must equal the reference BIT FOR BIT on every family, ring size and placement: the cases are exact in double
arithmetic (ring_cases.check_exact, asserted while the cases are built), so there is no tolerance and no case is filtered.

These tests pin the project's stated rule (the comment above closest_hit; ring_cases' module docstring).  shapely is not
available to them, so they make no new claim about how shapely itself reports a collinear overlap or a touching vertex: what
trajectory.py:83-129 does with shapely's answer -- keep the Point members of the intersection, drop everything else, take the
closest, fall back to the waypoint -- is what the rule was derived from."""
import numpy as np
import pytest

import ring_cases as rc
from oracle import oracle as orc

VARIANTS = {"strict": None, "fma": orc.fma_variant, "cr": orc.cr_variant}


def run_oracle(variant, pts, ring):
    out = pts.copy()
    if VARIANTS[variant] is None:
        return orc.fill_bounds(out, ring, ring, rc.MAX_DIST)
    with VARIANTS[variant]():
        return orc.fill_bounds(out, ring, ring, rc.MAX_DIST)


def test_exact_reference_on_hand_worked_cases():
    """The Fraction reference itself, on answers worked by hand: a unit square around the waypoint (tie to the lowest edge),
    a collinear edge, the range limit and no hit."""
    sq = [(-25.0, -40.0), (25.0, -40.0), (25.0, 40.0), (-25.0, 40.0)]
    assert rc.exact_closest_hit(0.0, 0.0, 100.0, 0.0, sq) == (rc.F(1, 4), 1)
    assert rc.exact_closest_hit(0.0, 0.0, 100.0, 0.0, sq[2:] + sq[:2]) == (rc.F(-1, 4), 1)
    assert rc.exact_closest_hit(0.0, 0.0, 100.0, 0.0, [(25.0, 0.0), (75.0, 0.0), (75.0, 40.0), (25.0, 40.0)]) == (rc.F(1, 4), 3)
    big = [(-100.0, -30.0), (100.0, -30.0), (100.0, 30.0), (-100.0, 30.0)]
    assert rc.exact_closest_hit(0.0, 0.0, 100.0, 0.0, big) == (rc.F(1), 1)
    assert rc.exact_closest_hit(0.5, 0.0, 100.0, 0.0, big) == (rc.F(199, 200), 1)
    assert rc.exact_closest_hit(200.5, 0.0, 100.0, 0.0, big) is None
    assert rc.exact_bound(200.5, 0.0, 100.0, 0.0, big) == (rc.F(401, 2), rc.F(0))
    assert rc.exact_closest_hit(0.0, 0.0, 0.0, 100.0, [(-1.0, 3.0), (1.0, 5.0), (1.0, 9.0), (-1.0, 9.0)]) == (rc.F(1, 25), 0)


def test_case_builder_covers_what_it_promises():
    """Every family at every size (g has no 4-vertex form), every placement target reached, nothing filtered: cases() asserts
    exactness and the families' expectations while it builds; here the counts."""
    n = 0
    for fam, nr in rc.GROUPS:
        cs = rc.cases(fam, nr)
        assert cs and all(len(c.ring) == nr and len(c.way) == len(c.hits) >= 1 for c in cs)
        n += len(cs)
    assert len(rc.GROUPS) == 9 * 6 - 1 and n >= 4 * len(rc.GROUPS)
    assert rc.cases("g", 4) == ()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("fam,nr", rc.GROUPS, ids=rc.GROUP_IDS)
def test_oracle_fill_bounds_is_exact(fam, nr, variant):
    for case in rc.cases(fam, nr):
        ring = rc.ring_array(case)
        for N, order in ((2 * len(case.way), "mono"), (65, "jump")):
            pts, side, exp = rc.table(case, N, order)
            out = run_oracle(variant, pts, ring)
            rc.assert_bits(rc.asserted(out, side), exp, f"{rc.describe(case)} {variant} N={N} {order}")
            keep = [c for c in range(19) if c not in (rc.LBX, rc.LBY, rc.RBX, rc.RBY)]
            rc.assert_bits(out[:, keep], pts[:, keep], f"{rc.describe(case)} {variant}: other columns")
