"""The shared-prefix planner (csrc/share_plan.hpp) through share_plan_sim: rows
given by their block chains (the block id of each leading tile; equal ids at a
depth mean equal pages up to it) and next positions, page_size 16.  Expected
groups follow the documented rule: greedy by saving (G - 1) * P, deeper on a
tie, one group per row, shared tiles strictly below every member's position."""
import pytest

import llm_capi

A = [1, 2, 3, 4]          # a four-tile header
B = [1, 2, 9]             # shares A's first two tiles
FAR = 1000                # a position past every chain


@pytest.mark.parametrize("name,chains,pos,min_pages,want", [
    # nested prefixes: three rows on A, two on the shorter B.  Saving of all five
    # at depth 2 is 4 * 2 = 8, of the A rows at depth 4 is 2 * 4 = 8: the tie goes
    # to the deeper candidate, then B's two rows share their three tiles
    ("nested", [A, B, A, A, B], [FAR] * 5, 1, [([0, 2, 3], 4), ([1, 4], 3)]),
    # row 2 could join all four rows at depth 1 (saving 3) or row 3 at depth 4
    # (saving 4): it goes where more reads are saved, and 0 and 1 still pair up
    ("either", [[1], [1], [1, 5, 6, 7], [1, 5, 6, 7]], [FAR] * 4, 1,
     [([2, 3], 4), ([0, 1], 1)]),
    # the minimum length: B's rows share only 3 tiles, A's share 4
    ("min_pages", [A, B, A, B], [FAR] * 4, 4, [([0, 2], 4)]),
    ("min_pages_none", [B, B], [FAR, FAR], 4, []),
    # a prefix reaching a member's current page: row 1 appends position 40, in
    # tile 2, so only tiles 0 and 1 are whole pages below it -- sharing 2 tiles
    # three ways (saving 4) beats sharing 4 tiles between rows 0 and 2 (also 4)
    # only on depth, so the deeper pair wins and row 1 stays alone
    ("current_page", [A, A, A], [FAR, 40, FAR], 1, [([0, 2], 4)]),
    # ... and at position 64 (tile 4) all four tiles are below it
    ("below_page", [A, A, A], [FAR, 64, FAR], 1, [([0, 1, 2], 4)]),
    ("off", [A, A], [FAR, FAR], 0, []),
])
def test_share_plan(name, chains, pos, min_pages, want):
    assert llm_capi.share_plan_sim(chains, pos, page_size=16, min_pages=min_pages) == want
