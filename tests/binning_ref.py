"""Plain numpy reference of the batched binning state of csrc/binning.hip.

Everything here is built from per-frame oracle.forward states (radii, means2D, depths,
tiles_touched) and the image size alone -- never from anything a GPU wrote, and not from the oracle's
own lists either: tests/test_binning_ref.py checks on the CPU that the ranges and lists derived here
reproduce the oracle's, tests/test_gpu_binning_state.py compares the GPU's workspace with them.

The contract (binning.hip's header): a frame's visible Gaussians are ordered by (depth bits, index);
the instances (Gaussian x tile of its rect) are emitted in that order, so tile t's list is the
subsequence of the order whose rect covers t.  The count table cuts the order into rows of `chunk`
Gaussians (helpers.chunk_rows) and holds, per row and tile, the instances of the rows before it.
"""
import numpy as np

import helpers

BLOCK = 16
DRAINED = 0xFFFFFFFF


def grid(W, H):
    return (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK


def rects(st, W, H):
    """getRect (auxiliary.h:45-55) of every Gaussian from the oracle state's means2D and radii, in
    float32 as there: int32 [P, 4] = x0, y0, x1, y1 (tile units, upper bounds exclusive)."""
    gx, gy = grid(W, H)
    m = np.ascontiguousarray(st["means2D"], np.float32)
    rf = st["radii"].astype(np.float32)
    s, one = np.float32(BLOCK), np.float32(1.0)

    def clamp(v, hi):
        return np.clip(np.trunc(v).astype(np.int64), 0, hi).astype(np.int32)
    out = np.stack([clamp((m[:, 0] - rf) / s, gx), clamp((m[:, 1] - rf) / s, gy),
                    clamp((((m[:, 0] + rf) + s) - one) / s, gx), clamp((((m[:, 1] + rf) + s) - one) / s, gy)], 1)
    out[st["radii"] <= 0] = 0
    return out


def frame_order(st):
    """Visible Gaussians by (depth bits, index): the stable argsort of the depth bits (as
    test_gpu_depth_sort._reference_order)."""
    idx = np.nonzero(st["tiles_touched"] > 0)[0]
    keys = np.ascontiguousarray(st["depths"], np.float32).view(np.uint32)[idx]
    return idx[np.argsort(keys, kind="stable")].astype(np.uint32)


def frame_reference(st, W, H):
    """One frame: order, rects, the count table rows it defines, tile counts, frame-local ranges and
    the list (Gaussian indices)."""
    gx, gy = grid(W, H)
    T = gx * gy
    chunk = helpers.chunk_rows(T)
    order = frame_order(st)
    V = len(order)
    rc = rects(st, W, H)
    w = (rc[:, 2] - rc[:, 0]).astype(np.int64)
    h = (rc[:, 3] - rc[:, 1]).astype(np.int64)
    assert ((w * h) == st["tiles_touched"].astype(np.int64)).all(), "rects disagree with the oracle's tiles_touched"
    n = (w * h)[order]                                   # instances per ordered Gaussian
    R = int(n.sum())
    owner = np.repeat(np.arange(V, dtype=np.int64), n)   # order position of every instance
    k = np.arange(R, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    ow = w[order][owner]
    dy = k // np.maximum(ow, 1)
    tile = (rc[order, 1][owner] + dy) * gx + rc[order, 0][owner] + (k - dy * ow)
    nrows = (V + chunk - 1) // chunk
    hist = np.bincount((owner // chunk) * T + tile, minlength=max(nrows, 1) * T).reshape(max(nrows, 1), T)[:nrows]
    table = (np.cumsum(hist, 0) - hist).astype(np.uint32)  # exclusive down the rows
    tile_count = np.bincount(tile, minlength=T).astype(np.uint32)
    ends = np.cumsum(tile_count.astype(np.int64))
    ranges = np.stack([ends - tile_count, ends], 1)
    ranges[tile_count == 0] = 0
    perm = np.argsort(tile, kind="stable")               # emission order kept inside every tile
    return dict(order=order, V=V, R=R, rects=rc, chunk=chunk, nrows=nrows, table=table, tile_count=tile_count,
                ranges=ranges, point_list=order[owner[perm]].astype(np.uint32),
                # ordered-scatter passes (kSlots Gaussians each) the row's workgroup takes
                passes=[-(-min(chunk, V - c * chunk) // helpers.SLOTS) for c in range(nrows)],
                full_grid=int(((w * h) == T).sum()))


def batch_reference(states, W, H):
    """B frames -> dict: frames (frame_reference each), fstat [B, 8] with the R / RBase / NonEmpty /
    Visible words filled, ctrl_R, ctrl_non_empty, tile_count [B*T], ranges [B*T, 2] shifted by each
    frame's RBase ((0, 0) for an empty tile) and the batch-wide point_list."""
    gx, gy = grid(W, H)
    T = gx * gy
    frames = [frame_reference(st, W, H) for st in states]
    B = len(frames)
    fstat = np.zeros((B, helpers.FS_WORDS), np.int64)
    base = 0
    ranges = np.zeros((B * T, 2), np.int64)
    for b, f in enumerate(frames):
        fstat[b, helpers.FS_R], fstat[b, helpers.FS_RBASE] = f["R"], base
        fstat[b, helpers.FS_NON_EMPTY] = int((f["tile_count"] > 0).sum())
        fstat[b, helpers.FS_VISIBLE] = f["V"]
        rg = f["ranges"] + base
        rg[f["tile_count"] == 0] = 0
        ranges[b * T:(b + 1) * T] = rg
        base += f["R"]
    return dict(frames=frames, B=B, T=T, gx=gx, gy=gy, chunk=frames[0]["chunk"], fstat=fstat, ctrl_R=base,
                ctrl_non_empty=int(fstat[:, helpers.FS_NON_EMPTY].sum()),
                tile_count=np.concatenate([f["tile_count"] for f in frames]),
                ranges=ranges.astype(np.uint32),
                point_list=np.concatenate([f["point_list"] for f in frames]) if B else np.zeros(0, np.uint32))


def lpt_hist(tile_count, B, T):
    """[B, 34]: tiles of each frame per work-list bucket."""
    out = np.zeros((B, helpers.LPT_BUCKETS), np.int64)
    for b in range(B):
        bk = [helpers.lpt_bucket(c) for c in tile_count[b * T:(b + 1) * T]]
        out[b] = np.bincount(bk, minlength=helpers.LPT_BUCKETS)
    return out


def strip_runs(tile_count, strip_max, B, T, gx):
    """Queue map 2's strip list layout from the tile counts and each tile's longest strip: the list is
    queue-major, bucket-major inside a queue's segment, frame-major inside a bucket.  Returns
    (offsets [B, 8, 129] -- the list position, in tiles, of the run of frame b's tiles of queue q and
    bucket k --, qstart [8], qcount [8])."""
    cnt = np.zeros((B, 8, helpers.STRIP_BUCKETS), np.int64)
    for tg in np.flatnonzero(tile_count):
        b, t = divmod(int(tg), T)
        cnt[b, int(helpers.tile_queue(t, gx)), helpers.strip_bucket(strip_max[tg])] += 1
    flat = cnt.transpose(1, 2, 0).reshape(-1)            # (queue, bucket, frame) order of the list
    off = (np.cumsum(flat) - flat).reshape(8, helpers.STRIP_BUCKETS, B).transpose(2, 0, 1)
    qcount = cnt.sum((0, 2))
    return off, np.cumsum(qcount) - qcount, qcount


def queue_item(q, k, ne, nempty, map_, ctrl):
    """gsr_internal.h queue_item: the k-th dequeue of queue q -- an item of [0, 4 ne) (strip_list
    position), of [4 ne, 4 ne + nempty) (empty tile work_list[ne + e]) or DRAINED."""
    if map_ == 0:
        item = q + 8 * k
        return item if item < 4 * ne + nempty else DRAINED
    if map_ == 2:
        nq = int(ctrl[helpers.CTRL_QSTART + 8 + q])
        if k < 4 * nq:
            return 4 * (int(ctrl[helpers.CTRL_QSTART + q]) + (k >> 2)) + (k & 3)
        e = q + 8 * (k - 4 * nq)
        return 4 * ne + e if e < nempty else DRAINED
    ntq = (ne - q + 7) >> 3 if ne > q else 0
    if k < 4 * ntq:
        return 4 * (q + 8 * (k >> 2)) + (k & 3)
    e = q + 8 * (k - 4 * ntq)
    return 4 * ne + e if e < nempty else DRAINED


def walk_queues(ne, nempty, map_, ctrl):
    """Every item the eight queues hand out, each queue walked from k = 0 until it is drained."""
    items = []
    for q in range(8):
        k = 0
        while True:
            it = queue_item(q, k, ne, nempty, map_, ctrl)
            if it == DRAINED:
                break
            items.append(it)
            k += 1
            assert k <= 4 * ne + nempty + 1, "a queue hands out more items than exist"
    return items


# ---------------------------------------------------------------- strip masks
#
# A point_list entry carries a 4-bit strip mask; a cleared bit s claims that no pixel of the tile's
# strip s (strip_origin: the 8x8 block at (16 tx + 8 (s % 2), 16 ty + 8 (s // 2))) reaches
# alpha >= 1/255.  The blend's own float32 rule decides (gsr_oracle.c: power by blend_power_m's fused
# form, skipped when > 0; alpha by gsro_blend_alpha).  Every (entry, pixel) pair is first evaluated in
# float64; a pair is settled there only when float32 rounding cannot move it across the threshold:
# |ln(255 alpha)| > BAND_REL + BAND_TERMS x (|A dx^2| + |B dx dy| + |C dy^2|) -- the power is six
# float32 operations on terms of those magnitudes (each within 2^-24 relative, 6 x 2^-24 < 4e-7), the
# exp restatement and the opacity product add a few 1e-7 relative -- and |power| likewise clear of the
# power > 0 skip.  Every other pair is evaluated by the oracle's own functions (libm fmaf, as
# gsr_oracle.c calls it, and oracle.blend_alpha), so no pair is left out.
BAND_REL, BAND_TERMS = 1e-3, 4e-7


def _fmaf():
    import ctypes
    import ctypes.util
    import oracle
    try:
        f = oracle.lib().fmaf
    except AttributeError:
        f = ctypes.CDLL(ctypes.util.find_library("m")).fmaf
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_float] * 3
    return f


def exact_reaches(co, dx, dy):
    """One pair by the oracle's float32 rule: conic_opacity row co, dx / dy = mean - pixel (float32)."""
    import oracle
    f = _fmaf()
    co = np.asarray(co, np.float32)
    dx, dy = np.float32(dx), np.float32(dy)
    A, Bb, Cq = np.float32(-0.5) * co[0], -co[1], np.float32(-0.5) * co[2]
    power = f(float(dy), f(float(Cq), float(dy), float(Bb * dx)), float((A * dx) * dx))
    if power > 0.0:
        return False
    return bool(oracle.blend_alpha(float(co[3]), [power])[0] >= np.float32(1.0) / np.float32(255.0))


def strip_reach(st, gidx, tiles, strips, W, H, exact_all=False):
    """For (entry, strip) pairs -- Gaussian gidx[i] in frame-local tile tiles[i], strip strips[i] --:
    bool [n, 8, 8] (y, x), whether the strip's pixel lies inside the image and takes the Gaussian
    (alpha >= 1/255) by the oracle's rule; the in-image pixels per pair; and the number of (entry,
    pixel) pairs settled by the oracle's own functions."""
    gx, _ = grid(W, H)
    strips = np.asarray(strips)
    co32 = np.ascontiguousarray(st["conic_opacity"], np.float32)[gidx]
    m32 = np.ascontiguousarray(st["means2D"], np.float32)[gidx]
    tx, ty = np.asarray(tiles) % gx, np.asarray(tiles) // gx
    px = (tx * BLOCK + (strips % 2) * 8)[:, None] + np.arange(8)[None, :]   # strip_origin
    py = (ty * BLOCK + (strips // 2) * 8)[:, None] + np.arange(8)[None, :]
    dx32 = m32[:, 0, None] - px.astype(np.float32)          # [n, 8] along x
    dy32 = m32[:, 1, None] - py.astype(np.float32)          # [n, 8] along y
    dx, dy = dx32.astype(np.float64)[:, None, :], dy32.astype(np.float64)[:, :, None]
    co = co32.astype(np.float64)
    A, Bb, Cq = (-0.5 * co[:, 0])[:, None, None], (-co[:, 1])[:, None, None], (-0.5 * co[:, 2])[:, None, None]
    t0, t1, t2 = A * dx * dx, Bb * dx * dy, Cq * dy * dy
    power = t0 + t1 + t2
    band = BAND_REL + BAND_TERMS * (np.abs(t0) + np.abs(t1) + np.abs(t2))
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        la = np.log(255.0 * co[:, 3])[:, None, None] + power  # ln(255 alpha)
    inside = (px < W)[:, None, :] & (py < H)[:, :, None]
    reach = (power <= 0.0) & (la >= 0.0)
    # far below the threshold no sign of the power matters; a NaN (which the blend takes: alpha 0.99)
    # goes to the oracle
    near = (((np.abs(la) <= band) | (np.abs(power) <= band)) & (la >= -band)) | np.isnan(la)
    if exact_all:
        near = np.ones_like(near)
    near &= inside
    idx = np.argwhere(near)
    for i, ly, lx in idx:
        reach[i, ly, lx] = exact_reaches(co32[i], dx32[i, lx], dy32[i, ly])
    return reach & inside, inside.sum((1, 2)), len(idx)


def strip_mask_audit(st, gidx, tiles, masks, W, H, step=100000, tight_cap=100000):
    """Soundness of the 4-bit strip masks of one frame's list: -> dict(cleared_pairs: in-image (entry,
    pixel) pairs under a cleared bit; violations: cleared bits whose strip holds a pixel that takes
    the Gaussian (bad: the first few, as (entry, strip)); exact_pairs: pairs settled by the oracle's own
    functions; skipped_pairs: pairs left out (none: see above); set_bits / idle_bits: over a sample
    of at most about tight_cap set bits, those with no pixel taking the Gaussian)."""
    masks = np.asarray(masks, np.int64)
    bits = (masks[:, None] >> np.arange(4)[None, :]) & 1       # [n, 4]
    out = dict(cleared_pairs=0, violations=0, exact_pairs=0, skipped_pairs=0, set_bits=0, idle_bits=0, bad=[])
    cleared = np.argwhere(bits == 0)                           # (entry, strip)
    for a in range(0, len(cleared), step):
        e, s = cleared[a:a + step, 0], cleared[a:a + step, 1]
        reach, npix, nexact = strip_reach(st, gidx[e], tiles[e], s, W, H)
        v = reach.any((1, 2))
        out["cleared_pairs"] += int(npix.sum())
        out["violations"] += int(v.sum())
        out["bad"] += [(int(e[i]), int(s[i])) for i in np.flatnonzero(v)[:4]]
        out["exact_pairs"] += nexact
    setb = np.argwhere(bits == 1)
    setb = setb[::max(1, -(-len(setb) // tight_cap))]
    for a in range(0, len(setb), step):
        e, s = setb[a:a + step, 0], setb[a:a + step, 1]
        reach, _, _ = strip_reach(st, gidx[e], tiles[e], s, W, H)
        out["set_bits"] += len(e)
        out["idle_bits"] += int((~reach.any((1, 2))).sum())
    return out
