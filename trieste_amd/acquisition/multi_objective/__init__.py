"""Multi-objective building blocks (reference trieste/acquisition/multi_objective/): the non-dominated filter, the Pareto
set with its hypervolume indicator, the partitions of the non-dominated region into cells, and the expected hypervolume
improvement of a point, and of a batch of points by Monte-Carlo, over a stack of engine-backed models.  The partitions are host arithmetic (numpy) on a few dozen front points;
the acquisition function itself runs on the device (tgp_ehvi_*, tgp_qehvi_*)."""
from .batch_ehvi import BatchMonteCarloExpectedHypervolumeImprovement, batch_ehvi, differentiable_batch_ehvi
from .dominance import non_dominated
from .ehvi import ExpectedHypervolumeImprovement, differentiable_expected_hv_improvement, expected_hv_improvement
from .pareto import Pareto, get_reference_point
from .partition import (DividedAndConquerNonDominated, ExactPartition2dNonDominated,
                        prepare_default_non_dominated_partition_bounds)
