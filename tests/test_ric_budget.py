"""The fence around the RIC kernels (ric_kernel.hip, prefix `nyxric_`, budgets in tests/golden/ric_budget.json) is the one of
tests/test_series_budget.py, family `ric`, which that file runs as its `[ric]` cases.  These three only keep the names the tests
had here, so that their records go on: nothing to add to when a family comes, and nothing is lost when they go."""
import test_series_budget as fence

pytestmark = fence.NEEDS


def test_every_ric_kernel_is_inside_its_budget():
    fence.test_every_kernel_is_inside_its_budget("ric")


def test_two_interpolations_per_sample_do_not_push_the_tables_into_scratch():
    fence.test_the_evaluation_kernel_does_not_push_the_interpolation_into_scratch("ric")


def test_ric_kernels_stay_out_of_the_other_fences():
    fence.test_the_kernels_stay_out_of_the_other_fences("ric")
