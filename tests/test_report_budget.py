"""The fence around the report kernels (report_kernel.hip, prefix `nyxrep_`, budgets in tests/golden/report_budget.json) is the one of
tests/test_series_budget.py, family `report`, which that file runs as its `[report]` cases.  These three only keep the names the tests
had here, so that their records go on: nothing to add to when a family comes, and nothing is lost when they go."""
import test_series_budget as fence

pytestmark = fence.NEEDS


def test_every_report_kernel_is_inside_its_budget():
    fence.test_every_kernel_is_inside_its_budget("report")


def test_the_parameter_block_does_not_push_the_interpolation_into_scratch():
    fence.test_the_evaluation_kernel_does_not_push_the_interpolation_into_scratch("report")


def test_report_kernels_stay_out_of_the_other_fence():
    fence.test_the_kernels_stay_out_of_the_other_fences("report")
