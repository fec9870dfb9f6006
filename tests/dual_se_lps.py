"""The exact reference of the dual simplex with steepest-edge pricing of the leaving row (``dual_pricing=1``), and the inputs of its
pivot-for-pivot tests (tests/test_dual_se_host.py, tests/test_gpu_dual_se.py).

``DualSteepestReference`` is ``dual_lps.DualReference`` with one thing changed, the choice of the leaving row: among the rows with
``x_i < 0`` the largest ``x_i^2 / beta_i``, ``beta_i`` the exact squared 2-norm of row i of its ``Fraction`` inverse; ties to the lowest
basic column, then the lowest row, as there.  The ratio test, the pivot and the bookkeeping are the inherited ``step``: it is run on
a copy of ``x`` in which every row but the chosen one is zero -- so the chosen row is the only infeasible one and the inherited rule
takes it -- and since the update of ``x`` is ``x_k -= theta alpha_k`` with ``theta`` from the chosen row alone, what that copy holds
afterwards is the change of every other row, and the new value of the chosen one.
"""
from fractions import Fraction

import dual_lps

# (seed, n_cuts) of the pivot-for-pivot cases at m = 5, 64 and 65 -- either side of one wave of rows -- chosen on the CPU
# (tests/test_dual_se_host.py checks them again) so that the reference alone meets dual_lps.assert_walk_conditions with
# MARGIN = 1e-6, makes at least 8 pivots (2 at m = 5) and, in at least one case, walks differently from dual_lps.DualReference.
# They are the children of dual_lps.WALK_CASES (8, 68 and 68 rows with their cuts), walked by the other rule.  Measured there: 4, 13
# and 9 pivots (largest infeasibility: 4, 16 and 12), smallest margins 0.073, 0.027 and 0.011, smallest infeasibilities 0.64, 0.0020
# and 0.0042; all three walks leave that of largest infeasibility at their first pivot.
SE_WALK_CASES = {5: (2005, 3), 64: (2064, 4), 65: (1065, 3)}


def row_norms(inverse):
    """The exact ``beta_i`` of every row of a ``Fraction`` inverse."""
    return [sum((v * v for v in row if v), Fraction(0)) for row in inverse]


class DualSteepestReference(dual_lps.DualReference):
    """``margins[k][0]`` is the relative lead of the chosen row's ``x_i^2 / beta_i`` over the runner-up's (1 where there is none)."""

    def leaving(self):
        """``(row, lead, smallest infeasibility)`` under the steepest-edge rule, or ``None`` where no row is infeasible."""
        beta = row_norms(self.inverse)
        keyed = sorted(((self.x[i] * self.x[i] / beta[i], -self.basis[i], -i) for i in range(self.m) if self.x[i] < 0), reverse=True)
        if not keyed:
            return None
        lead = 1.0 if len(keyed) == 1 else float((keyed[0][0] - keyed[1][0]) / keyed[0][0])
        return -keyed[0][2], lead, min(-self.x[i] for i in range(self.m) if self.x[i] < 0)

    def step(self):
        choice = self.leaving()
        if choice is None:
            return super().step()  # (no infeasible row: the inherited answer)
        p, lead, smallest = choice
        x, seen = self.x, self.smallest_infeasibility
        self.x = [v if i == p else Fraction(0) for i, v in enumerate(x)]
        reason = super().step()
        if reason is None:
            self.x = [v if i == p else x[i] + v for i, v in enumerate(self.x)]
            self.margins[-1] = (lead, self.margins[-1][1])
        else:
            self.x = x
        self.smallest_infeasibility = smallest if seen is None else min(seen, smallest)
        return reason
