"""The C ABI's refusals held to tests/golden/capi_refusals.json (tests/capi_refusals.py: the table
and how the golden file was recorded): the return value and the whole td_last_error() text of
every row, byte for byte.  The rows that need no handle run without a GPU; one GPU test replays the
whole table, which adds the full texts and the precedence of the refusals that need a handle."""
import pytest

import capi_refusals as R
from gym_TD import _lib


def _compare(got, want_ids):
    want = R.golden()
    assert list(got) == want_ids  # the rows that were to run ran, in table order
    bad = ["%s: got %r, recorded %r" % (rid, got[rid], want.get(rid)) for rid in want_ids if got[rid] != want.get(rid)]
    assert not bad, "\n".join(bad)


def test_golden_file_has_the_table_rows_and_no_others():
    assert list(R.golden()) == [r[0] for r in R.table()]


def test_every_entry_point_and_every_handle_has_rows():
    t = R.table()
    assert {r[1] for r in t} == {
        "td_step", "td_step_boards", "td_step_boards_dev", "td_copy_boards", "td_copy_boards_dev", "td_action_mask",
        "td_action_mask_boards", "td_action_mask_boards_dev", "td_set_step_kernel", "td_set_retained_step_kernel",
        "td_set_frame_skip", "td_set_obs_format", "td_sample_actions", "td_sample_actions_boards",
        "td_sample_actions_boards_dev"}
    assert {r[2] for r in t} == set(R.HANDLES) | {None}
    # no message with a source line (a HIP failure is no refusal); an accepted row has no message
    for rid, (rc, msg) in R.golden().items():
        assert (msg is None) == (rc >= 0), rid
        assert msg is None or ".hip:" not in msg, rid


def test_refusals_that_need_no_handle():
    _compare(R.replay(_lib, False), [r[0] for r in R.table() if r[2] is None])


@pytest.mark.gpu
def test_every_refusal_and_its_precedence_on_the_device():
    _compare(R.replay(_lib, True), [r[0] for r in R.table()])
