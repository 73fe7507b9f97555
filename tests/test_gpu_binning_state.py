"""The batched binning state of csrc/binning.hip, per element.

After a BatchRasterizer.forward the workspace is decoded (helpers.decode_batch_workspace) and every
table the binning leaves behind is compared with tests/binning_ref.py, which is built from the
oracle's per-frame state alone: the depth order, the (row x tile) count table, tile counts, ranges
with their per-frame base, the batch-wide point_list, the frame and control words; the strip masks
(strip_cnt is the popcount of the list's bits, and a cleared bit is sound by the oracle's own float32
blend rule on every pixel of the strip); the longest-first work list and its histogram; the strip
list of queue map 2 with its per-(frame, queue, bucket) offsets and segment bounds; the dispatch
walk of queue_item over the eight queues; and, after a backward, the backward's own tile-major strip
list.  Integer state is compared exactly, images, radii and inverse depth bit for bit.

Each case states the regime it is there for and asserts from the reference that it reaches it
(tests/binning_cases.py builds the scenes), then prints one regime line: V per frame, count-table
rows, scatter passes per row, full-grid splats and the share of (entry, pixel) pairs the strip-mask
audit left out (none: every pair near the threshold goes to the oracle's own functions).
"""
import numpy as np
import pytest
import torch

import binning_cases as bc
import binning_ref as br
import helpers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 32
SKIP_CAP = 1e-3  # largest share of cleared-bit pairs the strip audit may leave out


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def _args(case):
    sc, cams, B = case["sc"], case["cams"], case["B"]
    views = _t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = _t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = _t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    return [_t(case["means3D"]), _t(sc["colors"]), _t(sc["opacities"]), _t(sc["scales"]), _t(sc["rotations"]),
            views, projs, tanf, torch.zeros((B, C), device=DEV)]


def _forward(case, ref, counters=False):
    from guava_renderer_amd.batch import BatchRasterizer, render_counters
    r = BatchRasterizer(case["B"], case["P"], case["W"], case["H"], R_capacity=ref["ctrl_R"] + 1024, device=DEV)
    args = _args(case)
    for x in r.out_color, r.out_invdepth:
        x.fill_(7.0)
    r.radii.fill_(-7)
    cnt = None
    if counters:
        cnt = render_counters(lambda: r.forward(*args))
    else:
        r.forward(*args)
    torch.cuda.synchronize()
    assert not r.status()[1]
    return r, args, cnt


def _tile_groups(tag, lst, n_tiles):
    """A strip list of whole tiles: 4 consecutive entries per tile, strips 0..3 in order -> tile ids."""
    groups = np.asarray(lst[:4 * n_tiles], np.int64).reshape(n_tiles, 4)
    assert ((groups & 3) == np.arange(4)).all(), f"{tag}: a tile's strips are not consecutive in order 0..3"
    assert ((groups >> 2) == (groups[:, :1] >> 2)).all(), f"{tag}: a group of four mixes tiles"
    return groups[:, 0] >> 2


def _check_one_list(tag, tiles, nonempty, strip_max, T):
    """One longest-first tile-major list: every non-empty tile once, strip_bucket of the longest strip
    non-decreasing, frames ascending inside a bucket."""
    assert sorted(tiles.tolist()) == nonempty.tolist(), f"{tag}: not every non-empty tile exactly once"
    bk = np.array([helpers.strip_bucket(strip_max[t]) for t in tiles], np.int64)
    assert (np.diff(bk) >= 0).all(), f"{tag}: strip buckets decrease along the list"
    fr = tiles // T
    assert ((np.diff(fr) >= 0) | (np.diff(bk) > 0)).all(), f"{tag}: frames do not ascend inside a bucket"


def _check_dispatch(tag, ne, n_all, map_, ctrl, strip_list, work_list, nonempty, empty):
    """Walk queue_item over the eight queues: every strip of every non-empty tile once, every empty
    tile (through work_list[ne + e]) once, nothing else."""
    items = np.array(br.walk_queues(ne, n_all - ne, map_, ctrl), np.int64)
    assert len(items) == 4 * ne + (n_all - ne), f"{tag}: map {map_} hands out {len(items)} items"
    strips = np.sort(strip_list[items[items < 4 * ne]].astype(np.int64))
    np.testing.assert_array_equal(strips, (4 * nonempty[:, None] + np.arange(4)).reshape(-1),
                                  err_msg=f"{tag}: map {map_} strips")
    empt = np.sort(work_list[ne + (items[items >= 4 * ne] - 4 * ne)].astype(np.int64))
    np.testing.assert_array_equal(empt, empty, err_msg=f"{tag}: map {map_} empty tiles")


def _check_batch(tag, r, frames, ref, image_rows=None):
    """Everything the forward left in r's workspace against the reference `ref` of the oracle frames
    `frames` ((colour, radii, inverse depth, state) each).  image_rows: compare colour and inverse
    depth on these rows only (a slice).  Returns the decoded (image arena, lists) and the strip
    audit's totals."""
    B, P, W, H = r.B, r.P, r.W, r.H
    T, gx, chunk = ref["T"], ref["gx"], ref["chunk"]
    rows = slice(None) if image_rows is None else image_rows
    for b, (o_col, o_radii, o_inv, _) in enumerate(frames):
        np.testing.assert_array_equal(r.radii[b].cpu().numpy(), o_radii, err_msg=f"{tag}: radii {b}")
        np.testing.assert_array_equal(r.out_color[b, :, rows].cpu().numpy(), o_col[:, rows], err_msg=f"{tag}: colour {b}")
        np.testing.assert_array_equal(r.out_invdepth[b, rows].cpu().numpy(), o_inv.reshape(H, W)[rows],
                                      err_msg=f"{tag}: inverse depth {b}")
    gs, im, bn = helpers.decode_batch_workspace(r)
    ctrl = gs["ctrl"].astype(np.int64)
    fstat = ctrl[helpers.CTRL_WORDS:].reshape(B, helpers.FS_WORDS)
    # ---- control and frame words
    assert ctrl[1] == 0 and ctrl[helpers.CTRL_R] == ref["ctrl_R"] == bn["R"], (tag, ctrl[:8], ref["ctrl_R"])
    assert ctrl[helpers.CTRL_NON_EMPTY] == ref["ctrl_non_empty"], (tag, ctrl[helpers.CTRL_NON_EMPTY], ref["ctrl_non_empty"])
    for w in (helpers.FS_R, helpers.FS_RBASE, helpers.FS_NON_EMPTY, helpers.FS_VISIBLE):
        np.testing.assert_array_equal(fstat[:, w], ref["fstat"][:, w], err_msg=f"{tag}: frame word {w}")
    # ---- depth order and count table (rows the frame's visible Gaussians fill; the rest is unspecified)
    nchunk = -(-P // chunk)
    table = gs["table"].reshape(B, nchunk, T)
    for b, f in enumerate(ref["frames"]):
        np.testing.assert_array_equal(gs["order"].reshape(B, P)[b, :f["V"]], f["order"], err_msg=f"{tag}: order {b}")
        np.testing.assert_array_equal(table[b, :f["nrows"]], f["table"], err_msg=f"{tag}: table of frame {b}")
    # ---- tile counts, ranges, lists
    np.testing.assert_array_equal(im["tile_count"], ref["tile_count"], err_msg=f"{tag}: tile_count")
    np.testing.assert_array_equal(im["ranges"].reshape(B * T, 2), ref["ranges"], err_msg=f"{tag}: ranges")
    plist = bn["point_list"]
    np.testing.assert_array_equal(plist & helpers.INDEX_MASK, ref["point_list"], err_msg=f"{tag}: point_list")
    masks = (plist >> 28).astype(np.int64)
    # ---- strip masks: strip_cnt is the popcount of each bit over the tile's list ...
    tcount = ref["tile_count"].astype(np.int64)
    tile_of = np.repeat(np.arange(B * T), tcount)  # (the lists follow each other in tile order)
    assert (np.diff(ref["ranges"][tcount > 0].reshape(-1).astype(np.int64)) >= 0).all()
    want_cnt = np.zeros((B * T, 4), np.int64)
    for s in range(4):
        want_cnt[:, s] = np.bincount(tile_of, weights=(masks >> s) & 1, minlength=B * T)
    strip_cnt = im["strip_cnt"].reshape(B * T, 4).astype(np.int64)
    ne_mask = tcount > 0
    np.testing.assert_array_equal(strip_cnt, want_cnt, err_msg=f"{tag}: strip_cnt")
    # ... and a cleared bit is sound: no pixel of the strip takes the Gaussian (the oracle's rule)
    audit = dict(cleared_pairs=0, violations=0, exact_pairs=0, skipped_pairs=0, set_bits=0, idle_bits=0, bad=[])
    for b, f in enumerate(ref["frames"]):
        lo = int(ref["fstat"][b, helpers.FS_RBASE])
        a = br.strip_mask_audit(frames[b][3], f["point_list"], tile_of[lo:lo + f["R"]] - b * T,
                                masks[lo:lo + f["R"]], W, H)
        for k in audit:
            audit[k] += a[k] if k != "bad" else [(b,) + x for x in a[k]]
    assert audit["violations"] == 0, f"{tag}: cleared strip bits with a contributing pixel, (frame, entry, strip) {audit['bad'][:8]}"
    assert audit["skipped_pairs"] <= SKIP_CAP * max(audit["cleared_pairs"], 1)
    # ---- work list and its histogram
    work = im["work_list"].astype(np.int64)
    np.testing.assert_array_equal(im["lpt_hist"].reshape(B, helpers.LPT_BUCKETS), br.lpt_hist(tcount, B, T),
                                  err_msg=f"{tag}: lpt_hist")
    assert sorted(work.tolist()) == list(range(B * T)), f"{tag}: work_list is no permutation of the tiles"
    wb = np.array([helpers.lpt_bucket(tcount[t]) for t in work], np.int64)
    assert (np.diff(wb) >= 0).all(), f"{tag}: work_list buckets decrease"
    assert ((np.diff(work // T) >= 0) | (np.diff(wb) > 0)).all(), f"{tag}: work_list frames do not ascend inside a bucket"
    ne = ref["ctrl_non_empty"]
    nonempty, empty = np.flatnonzero(ne_mask), np.flatnonzero(~ne_mask)
    assert sorted(work[:ne].tolist()) == nonempty.tolist(), f"{tag}: work_list head is not the non-empty tiles"
    # ---- strip list
    strip_max = strip_cnt.max(1)
    lst = im["strip_list"]
    tiles = _tile_groups(tag, lst, ne)
    if B >= 2:  # queue map 2: per-queue segments, bucket-major, frames ascending inside a run
        off, qstart, qcount = br.strip_runs(tcount, strip_max, B, T, gx)
        np.testing.assert_array_equal(ctrl[helpers.CTRL_QSTART:helpers.CTRL_QSTART + 8], qstart, err_msg=f"{tag}: qstart")
        np.testing.assert_array_equal(ctrl[helpers.CTRL_QSTART + 8:helpers.CTRL_QSTART + 16], qcount, err_msg=f"{tag}: qcount")
        np.testing.assert_array_equal(im["strip_hist"].reshape(B, 8, helpers.STRIP_BUCKETS), off,
                                      err_msg=f"{tag}: strip_hist offsets")
        assert len(set(tiles.tolist())) == ne, f"{tag}: a tile is listed twice"
        for q in range(8):
            seg = tiles[qstart[q]:qstart[q] + qcount[q]]
            want = nonempty[helpers.tile_queue(nonempty % T, gx) == q]
            assert sorted(seg.tolist()) == want.tolist(), f"{tag}: queue {q}'s segment holds other tiles than its own"
            bk = np.array([helpers.strip_bucket(strip_max[t]) for t in seg], np.int64)
            assert (np.diff(bk) >= 0).all(), f"{tag}: queue {q}: buckets decrease inside the segment"
            assert ((np.diff(seg // T) >= 0) | (np.diff(bk) > 0)).all(), f"{tag}: queue {q}: frames do not ascend in a run"
            for b in range(B):  # each (frame, queue, bucket) run starts at its strip_hist offset
                for k in np.unique(bk[seg // T == b]):
                    first = int(np.flatnonzero((seg // T == b) & (bk == k))[0])
                    assert qstart[q] + first == off[b, q, k], (tag, q, b, int(k))
        _check_dispatch(tag, ne, B * T, 2, ctrl, lst, work, nonempty, empty)
    else:  # one frame: one longest-first list, walked tile-affine (map 1)
        _check_one_list(f"{tag}: strip_list", tiles, nonempty, strip_max, T)
        hist = np.bincount([helpers.strip_bucket(strip_max[t]) for t in nonempty], minlength=helpers.STRIP_BUCKETS)
        np.testing.assert_array_equal(im["strip_hist"][:helpers.STRIP_BUCKETS], hist, err_msg=f"{tag}: strip_hist")
        _check_dispatch(tag, ne, T, 1, ctrl, lst, work, nonempty, empty)
    return im, strip_max, nonempty, audit


def _check_backward_list(tag, r, args, im_fwd, strip_max, nonempty, ref):
    """One backward with helpers._bg_and_cotangents' cotangents: strip_list_bwd is one tile-major
    longest-first list over every non-empty tile, and the forward's lists are left as they were."""
    B, W, H, T = r.B, r.W, r.H, ref["T"]
    _, dL, dLinv = helpers._bg_and_cotangents(W, H)
    g = r.backward(*args, _t(np.repeat(dL[None], B, 0)), _t(np.repeat(dLinv, B, 0)))
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in g.values() if v is not None) and g["colors"].abs().max() > 0
    _, im, _ = helpers.decode_batch_workspace(r, geom=False)
    ne = len(nonempty)
    tiles = _tile_groups(f"{tag}: strip_list_bwd", im["strip_list_bwd"], ne)
    _check_one_list(f"{tag}: strip_list_bwd", tiles, nonempty, strip_max, T)
    for k in ("strip_list", "work_list", "strip_cnt", "ranges", "tile_count"):
        np.testing.assert_array_equal(im[k], im_fwd[k], err_msg=f"{tag}: the backward changed {k}")


def _regime_line(tag, case, ref, audit, cnt=None):
    rg = bc.regime(case, ref)
    skipped = audit["skipped_pairs"] / max(audit["cleared_pairs"], 1)
    idle = audit["idle_bits"] / max(audit["set_bits"], 1)
    print(f"  {tag}: V {rg['V']}, chunk {rg['chunk']}, nchunk {rg['nchunk']} (rows used {rg['rows']}), passes per row "
          f"{rg['passes']}, full-grid splats {rg['full_grid']}, R {rg['R']}; strip audit: {audit['cleared_pairs']} "
          f"cleared-bit pairs, {audit['exact_pairs']} settled by the oracle's functions, skipped share {skipped:.2g}; "
          f"set bits with no contributing pixel {idle:.3f} (of {audit['set_bits']} sampled)"
          + (f"; pairs evaluated {cnt['pairs_evaluated']}, contributing {cnt['pairs_contributing']}" if cnt else ""))
    return rg


def _check_counters(tag, cnt, case):
    """The exact statement of the masks' soundness: the instrumented kernel, which walks only the
    entries whose strip bit is set, evaluates and blends exactly the pairs the oracle's loop does."""
    import oracle
    visited = contrib = 0
    for f in case["frames"]:
        v, k = oracle.render_counts(f[3], case["W"], case["H"])
        visited += v
        contrib += k
    assert cnt["pairs_evaluated"] == visited and cnt["pairs_contributing"] == contrib, (tag, cnt, visited, contrib)


# ---------------------------------------------------------------- 1. ragged, an empty frame in the middle

@pytest.mark.parametrize("row", bc.ROW1, ids=[r[0] for r in bc.ROW1])
def test_ragged_batch_with_an_empty_middle_frame(row):
    """96x80 (ragged on both axes, T = 30), B = 3, frame 1 sees nothing.  256-Gaussian rows with V at
    slot and row boundaries (1, 64, 256, 257, 511, 512, 513); RBase is carried across the empty frame;
    nchunk * B is 3, 6 or 9, so the XCD-ordered scatter grid is padded to 8 or 16 workgroups and some
    find no item.  The B = 3 case with the most rows also runs the backward's list, the first the
    render counters."""
    tag = row[0]
    case = bc.make_case(*row[1:])
    ref = br.batch_reference(bc.states(case), case["W"], case["H"])
    a, b = row[6][0], row[6][2]
    # the regime, from the reference
    assert ref["chunk"] == 256 and ref["T"] == 30
    assert [f["V"] for f in ref["frames"]] == [a, 0, b]
    assert ref["fstat"][2, helpers.FS_RBASE] == ref["frames"][0]["R"] > 0 and ref["frames"][1]["R"] == 0
    N = -(-case["P"] // 256) * 3
    assert N in (3, 6, 9) and N % 8 != 0  # grid 8 * ceil(N / 8) > N: workgroups with item >= N
    counters = row is bc.ROW1[0] or row is bc.ROW1[5]
    r, args, cnt = _forward(case, ref, counters=counters)
    im, strip_max, nonempty, audit = _check_batch(tag, r, case["frames"], ref)
    if counters:
        _check_counters(tag, cnt, case)
    if row is bc.ROW1[5]:
        _check_backward_list(tag, r, args, im, strip_max, nonempty, ref)
    _regime_line(tag, case, ref, audit, cnt)


# ---------------------------------------------------------------- 2. T > 1024: the scatter's pass loop

@pytest.mark.parametrize("row", bc.ROW2, ids=[r[0] for r in bc.ROW2])
def test_multi_pass_scatter_batch(row):
    """528x512 (T = 1056 > 1024: 1024-Gaussian count rows, four scatter passes per row), B = 2 (the
    path whose base[] comes from the ranges), V at pass and row boundaries, scales x0.5 and two splats
    of scale 3.0 that cover all 1056 tiles.  Wherever a row takes four passes, some tile is hit by
    all four (base[] advanced three times on it)."""
    tag = row[0]
    case = bc.make_case(*row[1:])
    W, H = case["W"], case["H"]
    ref = br.batch_reference(bc.states(case), W, H)
    assert ref["chunk"] == 1024 and ref["T"] == 1056
    assert [f["V"] for f in ref["frames"]] == list(row[6])
    for f, v in zip(ref["frames"], row[6]):
        assert f["full_grid"] >= 2                                   # tiles_touched == T: k reaches T - 1
        last = ("partial" if v % 256 else "full") + ("+break" if f["passes"][-1] < 4 else "+count")
        assert last == bc.pass_loop_exit(v) and f["passes"][:-1] == [4] * (f["nrows"] - 1)
        if max(f["passes"]) == 4:
            assert _tile_hit_by_four_passes(f, ref["T"], ref["gx"]), f"{tag}: no tile takes instances from all four passes of a row"
    counters = row is bc.ROW2[0]
    r, args, cnt = _forward(case, ref, counters=counters)
    im, strip_max, nonempty, audit = _check_batch(tag, r, case["frames"], ref)
    if counters:
        _check_counters(tag, cnt, case)
    if row is bc.ROW2[-1]:
        _check_backward_list(tag, r, args, im, strip_max, nonempty, ref)
    _regime_line(tag, case, ref, audit, cnt)


def _tile_hit_by_four_passes(f, T, gx):
    """Whether some full row of the frame has a tile that receives instances from each of its four
    passes (from the reference's instance emission: order position -> pass, tile)."""
    rc, order = f["rects"], f["order"]
    for c, p in enumerate(f["passes"]):
        if p < 4:
            continue
        hit = np.ones(T, bool)
        for q in range(4):
            cover = np.zeros(T, bool)
            for g in order[c * 1024 + q * 256:c * 1024 + (q + 1) * 256]:
                x0, y0, x1, y1 = rc[g]
                cover.reshape(-1, gx)[y0:y1, x0:x1] = True
            hit &= cover
        if hit.any():
            return True
    return False


# ---------------------------------------------------------------- 3. one-tile-wide and one-tile-high grids

@pytest.mark.parametrize("row", bc.ROW3, ids=[r[0] for r in bc.ROW3])
def test_one_tile_wide_grids(row):
    """16x16400 and 16400x16 (T = 1025, gx = 1 / gy = 1), B = 2, P = 2000: k_chunk_count's 8-lane
    prefix sums see rows of two cells and columns of a thousand (and the transpose), the scatter's
    column / row ballots a single column (row); lists of a hundred tiles per Gaussian."""
    tag = row[0]
    case = bc.make_case(*row[1:])
    ref = br.batch_reference(bc.states(case), case["W"], case["H"])
    assert ref["T"] == 1025 and ref["chunk"] == 1024 and 1 in (ref["gx"], ref["gy"])
    assert [f["V"] for f in ref["frames"]] == list(row[6]) and min(f["R"] for f in ref["frames"]) > 100000
    r, args, cnt = _forward(case, ref)
    _, _, _, audit = _check_batch(tag, r, case["frames"], ref)
    _regime_line(tag, case, ref, audit)


# ---------------------------------------------------------------- 4. kMaxTiles: the > 64 KB LDS branches

@pytest.mark.parametrize("row", bc.ROW4, ids=[r[0] for r in bc.ROW4])
def test_largest_grids_single_frame_batch(row):
    """2048x2048 and 4096x1024 (T = 16384 = kMaxTiles), B = 1 through BatchRasterizer: both
    launch_chunk_count and launch_ordered_scatter ask for more than 64 KB of dynamic LDS,
    tile_scan_place_wg scans 64 tiles per thread inside the fused single-frame scatter (TS) at
    T > 1024, and one splat covers all 16384 tiles (ow = 128 and 256: the float k / ow at its largest
    operands).  Colour and inverse depth are compared on a 256-row band around the image centre (the
    radii and every state check cover the whole frame)."""
    tag = row[0]
    case = bc.make_case(*row[1:])
    W, H = case["W"], case["H"]
    ref = br.batch_reference(bc.states(case), W, H)
    gx, gy, T = ref["gx"], ref["gy"], ref["T"]
    assert T == helpers.MAX_TILES and T // helpers.SLOTS == 64 and ref["chunk"] == 1024
    assert (gx + 1) * (gy + 1) * 4 > 65536 and (gx + gy) * 32 + 4 * T > 65536
    f = ref["frames"][0]
    assert f["V"] == row[6][0] and f["full_grid"] >= 1
    full = np.flatnonzero(case["frames"][0][3]["tiles_touched"] == T)
    assert all(f["rects"][g][2] - f["rects"][g][0] == gx for g in full) and gx in (128, 256)
    r, args, cnt = _forward(case, ref)
    band = slice(H // 2 - 128, H // 2 + 128)
    _, _, _, audit = _check_batch(tag, r, case["frames"], ref, image_rows=band)
    _regime_line(tag, case, ref, audit)


# ---------------------------------------------------------------- 5. the drop-in single-frame entry

@pytest.mark.parametrize("row", bc.ROW5, ids=[r[0] for r in bc.ROW5])
def test_single_frame_entry_above_1024_tiles(row):
    """528x512 through the drop-in entry (helpers.gpu_forward, compared by test_gpu_forward's
    _compare_exact: ranges, lists, images), V = 1024, 1025, 2600: the fused single-frame TS scatter
    with 1024-Gaussian rows; then the count table, the frame words, the strip masks, the work list and
    the map-1 dispatch walk."""
    from test_gpu_forward import _compare_exact
    tag = row[0]
    case = bc.make_case(*row[1:])
    W, H = case["W"], case["H"]
    ref = br.batch_reference(bc.states(case), W, H)
    T, f = ref["T"], ref["frames"][0]
    assert T == 1056 and ref["chunk"] == 1024 and f["V"] == row[6][0] and f["full_grid"] >= 2
    d = dict(case["sc"])
    d["means3D"] = case["means3D"][0]
    d.update(case["cams"][0])
    d["bg"] = np.zeros(C, np.float32)
    gs, os_ = _compare_exact(d)
    np.testing.assert_array_equal(gs["ranges"].reshape(T, 2), ref["ranges"])
    np.testing.assert_array_equal(gs["point_list"][:gs["R"]], ref["point_list"])
    np.testing.assert_array_equal(gs["tile_count"], ref["tile_count"])
    np.testing.assert_array_equal(gs["order"][:f["V"]], f["order"])
    np.testing.assert_array_equal(gs["table"].reshape(-1, T)[:f["nrows"]], f["table"])
    ctrl = gs["ctrl"].astype(np.int64)
    tcount = ref["tile_count"].astype(np.int64)
    nonempty, empty = np.flatnonzero(tcount > 0), np.flatnonzero(tcount == 0)
    ne = len(nonempty)
    assert ctrl[helpers.CTRL_NON_EMPTY] == ne == ref["ctrl_non_empty"]
    work = gs["work_list"].astype(np.int64)
    assert sorted(work.tolist()) == list(range(T)) and sorted(work[:ne].tolist()) == nonempty.tolist()
    wb = np.array([helpers.lpt_bucket(tcount[t]) for t in work], np.int64)
    assert (np.diff(wb) >= 0).all()
    np.testing.assert_array_equal(gs["lpt_hist"], br.lpt_hist(tcount, 1, T)[0])
    fstat = ctrl[helpers.CTRL_WORDS:helpers.CTRL_WORDS + helpers.FS_WORDS]
    for w in (helpers.FS_R, helpers.FS_RBASE, helpers.FS_NON_EMPTY, helpers.FS_VISIBLE):
        assert fstat[w] == ref["fstat"][0, w], (tag, w, fstat, ref["fstat"][0])
    masks = gs["smask"][:gs["R"]].astype(np.int64)
    tile_of = np.repeat(np.arange(T), tcount)
    strip_cnt = gs["strip_cnt"].reshape(T, 4).astype(np.int64)
    for s in range(4):
        np.testing.assert_array_equal(strip_cnt[:, s], np.bincount(tile_of, weights=(masks >> s) & 1, minlength=T))
    audit = br.strip_mask_audit(os_, f["point_list"], tile_of, masks, W, H)
    assert audit["violations"] == 0, (tag, audit["bad"])
    assert audit["skipped_pairs"] <= SKIP_CAP * max(audit["cleared_pairs"], 1)
    strip_max = strip_cnt.max(1)
    tiles = _tile_groups(tag, gs["strip_list"], ne)
    _check_one_list(f"{tag}: strip_list", tiles, nonempty, strip_max, T)
    _check_dispatch(tag, ne, T, 1, ctrl, gs["strip_list"], work, nonempty, empty)
    _regime_line(tag, case, ref, audit)
