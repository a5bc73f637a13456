"""The reference of the spans tests (include/acgpu.h: acgpu_spans_*): the spans of a list of records through a coverage bitmap --
a difference array over the text's positions, its running sum, the boundaries of the covered runs.  Deliberately not the kernels'
algorithm (a suffix minimum and a prefix count over the records, csrc/acgpu_spans.hip).  A helper, not collected."""
import numpy as np


def merge(recs, n):
    """recs: (k, >= 2) records (start, end) in any order, 0 <= start < end <= n -> the (m, 2) int32 spans of a text of n positions:
    the maximal runs of positions that some record covers, ascending.  Touching records -- (1, 5) and (5, 8) -- cover positions
    that are consecutive, so they fall into one span."""
    recs = np.asarray(recs, dtype=np.int64)
    recs = recs.reshape(len(recs), -1)[:, :2] if recs.size else np.zeros((0, 2), np.int64)
    diff = np.zeros(n + 2, dtype=np.int64)
    np.add.at(diff, recs[:, 0] + 1, 1)
    np.add.at(diff, recs[:, 1] + 1, -1)
    covered = np.cumsum(diff) > 0  # covered[p + 1]: position p is covered; covered[0] and covered[n + 1] never are
    edges = np.flatnonzero(covered[1:] != covered[:-1])  # position p where coverage changes between p - 1 and p
    return edges.reshape(-1, 2).astype(np.int32)
