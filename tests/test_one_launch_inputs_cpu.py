"""The inputs of tests/test_gpu_one_launch_edges.py, checked without a device: every case of tests/small_edges.py is built and its
reach assertions run against the CPU oracle -- the record lists at 4095, 4096 and 4097 occurrences, keywords of 255, 256 and 257
units across the lane seams, the Longest chain whose only match is the last unit, the WholeWord runs on the seams and the text's
ends, U+0000 at the end of the text.  An edit of an input that takes it off its edge fails here."""
import numpy as np
import pytest

from tests import small_edges as E


@pytest.mark.parametrize("group", list(E.GROUPS))
def test_every_case_reaches_its_edge(group):
    cases = E.GROUPS[group]()  # (the reach assertions of the group run inside)
    assert cases and len({(c.name, c.mode) for c in cases}) == len(cases)
    for c in cases:
        n = c.hay.size
        assert c.recs.ndim == 2 and c.recs.shape[1] == 3 and c.hay.dtype == np.uint16
        assert len(c.recs) == 0 or (c.recs[:, 0] >= 0).all() and (c.recs[:, 0] < c.recs[:, 1]).all() and (c.recs[:, 1] <= n).all()
        assert c.one_launch == (c.why is None)


def test_the_refused_calls_are_the_ones_the_gate_names():
    """Across the groups: exactly the five kinds of call the one launch hands on, each for its own reason."""
    refused = {}
    for group in E.GROUPS.values():
        for c in group():
            if not c.one_launch:
                refused.setdefault(c.why, set()).add(c.name)
    assert refused == {"records": {"a_4097"}, "max_len": {"b_257", "b_257_alone"}, "fold": {"e_fold_inconsistent"},
                       "family": {"e_wwlongest"}, "units": {"e_4097_units"}}


def test_the_lengths_cover_both_sides_of_every_power_of_two_the_doubling_ends_on():
    """`for (span = 1; span < n; span <<= 1)`: n = 2^k needs k rounds, 2^k + 1 one more, 2^k - 1 the same k."""
    rounds = {n: int(np.ceil(np.log2(n))) if n > 1 else 0 for n in E.D_LENGTHS}
    assert rounds == {1: 0, 2: 1, 3: 2, 1023: 10, 1024: 10, 1025: 11, 4095: 12, 4096: 12}
