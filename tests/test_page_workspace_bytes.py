"""The workspace sizes of the page-analysis entries against recorded values: rtn_cca_workspace_bytes, rtn_lattice_workspace_bytes,
rtn_header_workspace_bytes, rtn_visual_effect_workspace_bytes, rtn_resize_u8_workspace_bytes, rtn_skew_workspace_bytes,
rtn_render_workspace_bytes and the offsets of rtn_skew_counts_layout.  tests/golden/page_workspace_bytes.json holds the argument
sets (n = 0, one 30 x 30 page, mixed sizes, the side limits, rejected arguments that give 0) beside the results, recorded from a
build of commit 55af84a ("Table structure on the device: rows, columns and cells of each table"), the last one whose entries
computed their layouts by hand; the table stager of csrc/rtn_page_launch.h must give the same numbers."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "page_workspace_bytes.json")


def call(lib, fn, args):
    """fn over the JSON arguments (a list is an int32 table, null a missing one).  rtn_skew_counts_layout gives
    {"rc": code, "offsets": its n offsets when rc is 0}; it is given room for them whatever n says."""
    keep = [np.ascontiguousarray(a, np.int32) if isinstance(a, list) else a for a in args]
    raw = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep]
    if fn != "rtn_skew_counts_layout":
        return int(getattr(lib, fn)(*raw))
    n = max(int(args[0]), 0)
    offsets = np.full(max(n, 1), -1, np.int64)
    rc = int(lib.rtn_skew_counts_layout(*raw, offsets.ctypes.data))
    return {"rc": rc, "offsets": [int(v) for v in offsets[:n]] if rc == 0 else []}


with open(GOLDEN) as f:
    RECORDS = json.load(f)


def test_the_record_covers_every_size_function():
    assert len(RECORDS) >= 40
    assert {r["fn"] for r in RECORDS} == {"rtn_cca_workspace_bytes", "rtn_lattice_workspace_bytes", "rtn_header_workspace_bytes",
                                           "rtn_visual_effect_workspace_bytes", "rtn_resize_u8_workspace_bytes",
                                           "rtn_skew_workspace_bytes", "rtn_render_workspace_bytes", "rtn_skew_counts_layout"}


@pytest.mark.parametrize("k", range(len(RECORDS)), ids=["%s-%d" % (r["fn"][4:], k) for k, r in enumerate(RECORDS)])
def test_size_equals_the_recorded_value(pkg, k):
    r = RECORDS[k]
    assert call(pkg.lib, r["fn"], r["args"]) == r["result"], r
