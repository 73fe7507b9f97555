"""tests/binning_ref.py against the oracle, on the CPU.

The reference derives ranges and lists from the depth order and the rects alone; on two small scenes
(a ragged 96x80 batch with an empty frame between two live ones, and a 528x512 frame with T > 1024,
1024-Gaussian table rows and two full-grid splats) they must reproduce the oracle's own per-frame
ranges and lists, the table must be the running per-tile count of the rows, and the float64 shortcut
of the strip-mask audit must agree with the oracle's float32 rule on every single pair.
"""
import numpy as np
import pytest

import binning_cases as bc
import binning_ref as br
import helpers

SMALL = [bc.ROW1[3], ("528x512-V1025-300", 528, 512, 1065, 60, 0.5, (1025, 300), (3.0, 3.0))]


@pytest.mark.parametrize("row", SMALL, ids=[r[0] for r in SMALL])
def test_reference_reproduces_the_oracle(row):
    case = bc.make_case(*row[1:])
    W, H, B = case["W"], case["H"], case["B"]
    states = bc.states(case)
    ref = br.batch_reference(states, W, H)
    T = ref["T"]
    assert [f["V"] for f in ref["frames"]] == list(case["V"])  # the case builder's V is the oracle's
    base = 0
    for b, (st, f) in enumerate(zip(states, ref["frames"])):
        assert f["R"] == st["R"]
        np.testing.assert_array_equal(f["ranges"], st["ranges"])
        np.testing.assert_array_equal(f["point_list"], st["point_list"])
        # batch-wide: the oracle's range shifted by the instances of the frames before it
        want = st["ranges"].astype(np.int64) + base
        want[st["ranges"][:, 1] == st["ranges"][:, 0]] = 0
        np.testing.assert_array_equal(ref["ranges"][b * T:(b + 1) * T], want)
        np.testing.assert_array_equal(ref["point_list"][base:base + f["R"]], st["point_list"])
        assert ref["fstat"][b, helpers.FS_RBASE] == base
        base += f["R"]
        # table: row c holds, per tile, the list entries whose Gaussian sits in the order rows before c
        pos = np.full(case["P"], -1, np.int64)
        pos[f["order"]] = np.arange(f["V"])
        assert f["table"].shape == (-(-f["V"] // f["chunk"]), T)
        for t in range(T):
            s, e = st["ranges"][t]
            rows_of = pos[st["point_list"][s:e]] // f["chunk"]
            assert (np.diff(rows_of) >= 0).all()
            np.testing.assert_array_equal(f["table"][:, t], np.searchsorted(rows_of, np.arange(f["nrows"])))
        assert (f["tile_count"] == st["ranges"][:, 1] - st["ranges"][:, 0]).all()
    assert ref["ctrl_R"] == base
    assert ref["ctrl_non_empty"] == int((ref["tile_count"] > 0).sum())
    np.testing.assert_array_equal(br.lpt_hist(ref["tile_count"], B, T).sum(1), np.full(B, T))


def test_queue_item_walks_cover_every_item_once():
    """queue_item on synthetic control words: maps 1 and 2 hand out every strip item and every empty
    tile exactly once."""
    ctrl = np.zeros(64, np.int64)
    qcount = np.array([3, 0, 5, 1, 0, 0, 7, 2])
    ctrl[helpers.CTRL_QSTART:helpers.CTRL_QSTART + 8] = np.cumsum(qcount) - qcount
    ctrl[helpers.CTRL_QSTART + 8:helpers.CTRL_QSTART + 16] = qcount
    ne = int(qcount.sum())
    for map_, nempty in ((2, 0), (2, 13), (1, 0), (1, 13), (0, 5)):
        items = br.walk_queues(ne, nempty, map_, ctrl)
        assert sorted(items) == list(range(4 * ne + nempty)), (map_, nempty)
    assert br.walk_queues(0, 0, 2, np.zeros(64, np.int64)) == []


def test_bucket_functions():
    assert [helpers.lpt_bucket(c) for c in (0, 1, 2, 3, 4, 2 ** 31)] == [33, 31, 30, 30, 29, 0]
    assert [helpers.strip_bucket(c) for c in (0, 1, 2, 3, 4, 5, 7, 8)] == [128, 127, 123, 121, 119, 118, 116, 115]
    b = [helpers.strip_bucket(c) for c in range(1, 5000)]
    assert all(x >= y for x, y in zip(b, b[1:])) and min(b) >= 0
    assert int(helpers.tile_queue(0, 7)) == 0 and int(helpers.tile_queue(4 * 7 + 4, 7)) == 4


def test_strip_audit_shortcut_equals_the_oracle_rule_on_every_pair():
    """strip_reach settles most pairs in float64 and hands the rest to the oracle's functions; with
    exact_all every pair goes to the oracle.  Both must give the same booleans (so the audit leaves no
    pair out: its skipped share is 0 <= the 1e-3 cap on every scene), and the audit must flag a mask
    with a wrongly cleared bit and accept the exact masks."""
    case = bc.make_case(*bc.ROW1[1][1:])  # 96x80, V = 64 / 0 / 256
    W, H = case["W"], case["H"]
    st = bc.states(case)[0]
    f = br.frame_reference(st, W, H)
    tiles = np.repeat(np.arange(len(f["tile_count"])), f["tile_count"])
    gidx = f["point_list"]
    e, s = np.repeat(np.arange(len(gidx)), 4), np.tile(np.arange(4), len(gidx))
    fast, _, nexact = br.strip_reach(st, gidx[e], tiles[e], s, W, H)
    slow, _, nall = br.strip_reach(st, gidx[e], tiles[e], s, W, H, exact_all=True)
    np.testing.assert_array_equal(fast, slow)
    assert nexact < nall // 20 and fast.any() and not fast.all()
    exact = (fast.any((1, 2)).reshape(-1, 4) << np.arange(4)).sum(1)
    a = br.strip_mask_audit(st, gidx, tiles, exact, W, H)
    assert a["violations"] == 0 and a["idle_bits"] == 0 and a["cleared_pairs"] > 0 and a["skipped_pairs"] == 0
    assert a["set_bits"] == int(sum(bin(int(m)).count("1") for m in exact))
    wrong = exact.copy()
    i = int(np.flatnonzero(exact)[0])
    wrong[i] &= wrong[i] - 1  # clear its lowest set bit
    bad = br.strip_mask_audit(st, gidx, tiles, wrong, W, H)
    assert bad["violations"] == 1 and bad["bad"][0][0] == i


def test_pass_loop_cases_cover_every_exit():
    """(Arithmetic only.)  The V list of the T > 1024 batch cases of tests/test_gpu_binning_state.py takes
    every exit of the ordered scatter's pass loop, and the 96x80 cases every padded grid size."""
    got = {bc.pass_loop_exit(v) for row in bc.ROW2 for v in row[6]}
    assert got == {"partial+break", "full+break", "partial+count", "full+count"}, got
    assert {-(-row[3] // 256) * 3 for row in bc.ROW1} == {3, 6, 9}
