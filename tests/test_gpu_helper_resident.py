"""GPU: the resident feed of the helpers' column walk (`Tuning.helper_resident`; pk_cooperative.h, helper_body; pk_harmonics.h,
harmonics_resident).  A helper workgroup of the plain sixteen-wave kernel copies the table rows of its columns into LDS once per launch
and walks them from there: the same nine f64 operations per row on the same operands in the same order as the scalar feed, so states
and statistics must be equal bit for bit - for part-filled owners, helper columns that are no multiple of a sixteen-row group or
shorter than one, waves with two columns, and when an owner gives up on its helper and walks the columns itself.  Where the block does
not fit (or the launch has no claim-mode helpers) the old feed runs, and the context says which one ran.

Every case is a process of its own (tests/helper_resident_cases.py) under a time limit of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 120  # context creation included; the kernels themselves take well under a second


def run_case(case):
    r = subprocess.run([sys.executable, os.path.join(HERE, "helper_resident_cases.py"), case], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    print(res)
    assert res["ok"], res
    assert all(res["equal"].values()), res   # states, epochs, status, accepted / rejected steps, evaluations: bit for bit
    assert all(res["twin_equal"]), res       # (the accounting twin of the kernel, which counts the jobs below: the same bits again)
    return res


def walked_from_lds(res):
    """The device's own word on the feed: every helper job of the resident run was walked from LDS, none of the other run's."""
    return res["jobs"][0] > 0 and res["lds_jobs"][0] == res["jobs"][0] and res["jobs"][1] > 0 and res["lds_jobs"][1] == 0


@pytest.mark.parametrize("case", ["deg70_n700", "deg70_n192", "deg40_n520", "deg24_n520"])
def test_resident_feed_matches_scalar_feed(case):
    """Claim-mode helpers, resident (2) against scalar (0): 11 owners with the last one part-filled at degree 70; the smallest
    claim-mode launch (three owners, nine helpers); columns that are no multiple of sixteen rows (degree 40) and shorter than a
    group (degree 24).  The context reports the feeds, and the device confirms them job for job."""
    res = run_case(case)
    assert res["helpers"][0] > 0 and res["helpers"][0] == res["helpers"][1]
    assert res["feed"] == [2, 0], res
    assert walked_from_lds(res), res


def test_single_owner():
    """64 trajectories: one owner.  It cannot have resident helpers - the claim mode wants at least eight helper workgroups and deals
    at most three per owner, so a single owner cooperates in the fan-out mode, whose kernel keeps its feed: this case pins that the
    new field changes nothing there (both runs walk with the old feed, no job from LDS); the resident walk with few owners is
    `deg70_n192` above."""
    res = run_case("deg70_n64")
    assert res["helpers"][0] > 0 and res["helpers"][0] == res["helpers"][1]
    assert res["feed"][0] == res["feed"][1] != 2 and res["lds_jobs"] == [0, 0], res


def test_owner_fallback_with_the_resident_feed_selected():
    """Helpers that never answer: the owners time out, walk the helper's columns with their own feed and finish alone - the same bits
    whether the launch was planned with the resident feed or not."""
    res = run_case("fallback_deg70_n700")
    assert res["helpers"][0] > 0 and res["feed"] == [2, 0] and res["lds_jobs"] == [0, 0], res  # (muted helpers take no job)


@pytest.mark.parametrize("case,helpers", [("nofit_deg150_n128", False), ("nofit_deg150_n512", True)])
def test_block_that_does_not_fit_keeps_the_old_feed(case, helpers):
    """150x150: 128 trajectories are two owners, too few for helpers at all; 512 with a one-part hand-off give every helper 168 KB of
    rows.  Neither stages anything, and the context reports the feed that ran (1 = streamed, the helpers' feed above degree 95)."""
    res = run_case(case)
    assert res["feed"][0] == res["feed"][1] == (1 if helpers else -1), res
    assert (res["helpers"][0] > 0) == helpers and res["helpers"][0] == res["helpers"][1]
    assert res["lds_jobs"] == [0, 0] and (res["jobs"][0] > 0) == helpers, res
