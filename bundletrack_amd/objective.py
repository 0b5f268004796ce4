"""The objective report on the MI355X: the cost the Gauss-Newton loop descends, at given poses (btba_objective_batch_zn_aux).

BatchSolver.objective_zn returns the instance totals and the per-pair records (include/btba.h: btba_objective_total, btba_objective_pair).  What a
caller of pose_covariances is missing -- a residual variance to scale the solver's matrix by -- follows from the totals: residual_variance."""
from __future__ import annotations

import numpy as np

from ._lib import OBJECTIVE_PAIR_DTYPE, OBJECTIVE_TOTAL_DTYPE      # noqa: F401  (the record layouts, for callers that take the device tensors)


def residual_variance(total, n_frames: int):
    """objective / (n_residuals - 6 (n_frames - 1)): the cost per degree of freedom left once the 6 (n_frames - 1) unknowns are spent (frame 0
    is fixed).  total: the structured array objective_zn returns (or one element of it); NaN where the denominator is not positive."""
    t = np.asarray(total)
    dof = t["n_residuals"].astype(np.float64) - 6.0 * (int(n_frames) - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dof > 0, t["objective"] / np.where(dof > 0, dof, 1.0), np.nan)
