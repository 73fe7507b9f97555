"""The per-frame depth sort of binning.hip at the bucket sizes and ties the other scenes never reach.

Every forward's per-tile list order comes from one stable sort of the frame's visible Gaussians by
(depth bits, index) (DESIGN.md §3 rule 5).  Buckets of at most kTinyBucket = 64 keys are ranked in
place (k_bucket_rank); larger ones go to k_bucket_sort, which ranks by sub-bucket in LDS, falls back
to an LDS bitonic network when a sub-bucket holds more than 48 keys (ties), and sorts buckets above
kSortLargeCap = 8192 keys with a bitonic network in global memory; the batched launch splits them
between a 256-thread (<= 2048 keys) and a 1024-thread kernel.  The scenes here (helpers.depth_cloud)
collapse the depth range or repeat depths exactly so that each of those paths sorts real buckets.

Each case is compared with the oracle bit-exactly (images, lists, ranges: _compare_exact), and the
decoded geometry arena is checked per frame: order[:V] is the stable argsort of the oracle's depth
bits over its visible Gaussians, the bucket-start table is a monotone partition of that order with
equal keys sharing a bucket, the worklist counts exactly the buckets above 64, and the counts slab
still holds the counts (the single-frame scatter scans them in every workgroup, so nothing may
overwrite them).  Each case states the sort paths it is there for; the path of every large bucket is
derived from the GPU's own table and a case that does not reach its paths fails.
"""
import numpy as np
import pytest

import helpers
from helpers import depth_cloud, depth_scene
from test_gpu_forward import _compare_exact

pytestmark = pytest.mark.gpu

kDegenerate = 48  # sort_segment_lds: a sub-bucket above this sends the segment to the LDS bitonic


def _reference_order(os_):
    """The contract: visible Gaussians by (depth bits, index).  Returns (indices, their keys)."""
    idx = np.nonzero(os_["tiles_touched"] > 0)[0]
    keys = np.ascontiguousarray(os_["depths"], np.float32).view(np.uint32)[idx]
    o = np.argsort(keys, kind="stable")
    return idx[o].astype(np.uint32), keys[o]


def _sub_bucket_max(ks):
    """sort_segment_lds' sub-bucket of each key of one sorted segment (float32 arithmetic as there):
    the largest sub-bucket's population."""
    n = len(ks)
    scale = np.float32(n) / (np.float32(ks[-1] - ks[0]) + np.float32(1.0))
    bb = np.minimum(((ks - ks[0]).astype(np.float32) * scale).astype(np.uint32), np.uint32(n - 1))
    return int(np.bincount(bb).max())


def _path(ks, batched):
    """Which code of k_bucket_sort sorts a large bucket holding the (sorted) keys ks."""
    n = len(ks)
    if n > helpers.SORT_LARGE_CAP:
        p = "global_bitonic"
    else:
        p = "lds_bitonic" if _sub_bucket_max(ks) > kDegenerate else "lds_rank"
    if batched:
        p = ("256:" if n <= helpers.SORT_SMALL_CAP else "1024:") + p
    return p


def _check_frame(tag, os_, order, bcount, bstart, fstat, batched):
    """One frame's sort state against the oracle; returns (bucket sizes, {path: sizes of its buckets})."""
    ref, ks = _reference_order(os_)
    V, NB = len(ref), len(bstart) - 1
    assert int(fstat[helpers.FS_VISIBLE]) == V, (tag, int(fstat[helpers.FS_VISIBLE]), V)
    np.testing.assert_array_equal(order[:V], ref, err_msg=f"{tag}: order")
    st = bstart.astype(np.int64)
    assert st[0] == 0 and st[NB] == V and (np.diff(st) >= 0).all(), tag
    cuts = np.unique(st[1:NB])
    cuts = cuts[(cuts > 0) & (cuts < V)]  # where one non-empty bucket ends and the next begins
    assert (ks[cuts - 1] < ks[cuts]).all(), f"{tag}: a bucket boundary splits equal keys or inverts the order"
    sizes = np.diff(st)
    # the counts slab is never scanned in place (the fused single-frame scatter reads it from every workgroup)
    np.testing.assert_array_equal(bcount[:NB], sizes, err_msg=f"{tag}: counts slab")
    assert bcount[NB] == 0, tag
    paths = {}
    big = np.nonzero(sizes > helpers.TINY_BUCKET)[0]
    for k in big:
        seg = ks[st[k]:st[k + 1]]
        paths.setdefault(_path(seg, batched), []).append((len(seg), len(np.unique(seg))))
    tiny = sizes[(sizes > 0) & (sizes <= helpers.TINY_BUCKET)]
    print(f"  {tag}: V {V} of {len(os_['depths'])}, NB {NB}, {len(big)} big, {len(tiny)} tiny (largest "
          f"{int(tiny.max(initial=0))}); (keys, distinct) by path: "
          + "; ".join(f"{p} {sorted(v, reverse=True)[:4]}{'...' if len(v) > 4 else ''} x{len(v)}"
                      for p, v in sorted(paths.items())))
    return sizes, paths


def _assert_regime(tag, paths, need):
    """need: {path: least number of buckets}; a path not named must not occur."""
    got = {p: len(v) for p, v in paths.items()}
    for p, n in need.items():
        assert got.get(p, 0) >= n, f"{tag}: wants {n} bucket(s) on {p}, has {got}"
    assert set(got) <= set(need), f"{tag}: unexpected paths {got}, wants {need}"


def _single(tag, d, need):
    gs, os_ = _compare_exact(d)
    fstat = gs["ctrl"][helpers.CTRL_WORDS:helpers.CTRL_WORDS + helpers.FS_WORDS]
    sizes, paths = _check_frame(tag, os_, gs["order"], gs["bcount"], gs["bstart"], fstat, batched=False)
    nbig = int((sizes > helpers.TINY_BUCKET).sum())
    assert int(gs["ctrl"][helpers.CTRL_NUM_BIG]) == nbig, (tag, int(gs["ctrl"][helpers.CTRL_NUM_BIG]), nbig)
    NB = len(sizes)
    assert sorted(gs["big"][:nbig].tolist()) == np.nonzero(sizes > helpers.TINY_BUCKET)[0].tolist(), tag
    assert NB == helpers._nb(d["means3D"].shape[0])
    _assert_regime(tag, paths, need)
    return sizes, paths


# ---------------------------------------------------------------- single frame

def test_plane_64_ranked_in_place_65_sorted():
    """All keys tied in one bucket: 64 keys are still k_bucket_rank's (the worklist stays empty),
    65 are the first size k_bucket_sort takes -- all tied, so one sub-bucket of 65 > 48: LDS bitonic."""
    sizes, _ = _single("plane 64", depth_scene(64, 31, "plane"), {})
    assert sizes.max() == 64 and sizes.sum() == 64
    sizes, paths = _single("plane 65", depth_scene(65, 32, "plane"), {"lds_bitonic": 1})
    assert paths["lds_bitonic"] == [(65, 1)]


@pytest.mark.parametrize("P,small,path", [(2048, 0.3, "lds_bitonic"), (2049, 0.3, "lds_bitonic"),
                                          (8192, 0.2, "lds_bitonic"), (8193, 0.2, "global_bitonic"),
                                          (20000, 0.15, "global_bitonic")])
def test_plane_one_tied_bucket(P, small, path):
    """One bucket of exactly P tied keys (nothing culled): the LDS bitonic up to its 8192-key cap, the
    global-memory bitonic from 8193, at powers of two, one past them, and far from one (20000: 12768
    virtual +inf pads).  The sorted order is the identity here, and only a correct network finds it."""
    _, paths = _single(f"plane {P}", depth_scene(P, 40 + P % 7, "plane", small=small), {path: 1})
    assert paths[path] == [(P, 1)]


def test_plane_culled_ties_with_index_gaps():
    _, paths = _single("plane 3000 culled", depth_scene(3000, 33, "plane", culled=0.2), {"lds_bitonic": 1})
    (n, distinct), = paths["lds_bitonic"]
    assert 2000 < n < 2800 and distinct == 1


def test_outliers_lds_rank_path():
    """Two outliers stretch the key range: the cloud falls into a dozen buckets of several hundred
    mostly distinct keys, each ranked by sub-bucket in LDS."""
    d = depth_scene(10000, 34, "squeeze", W=128, H=96, zspread=1.0, outliers=True, culled=0.2)
    _, paths = _single("outliers 10k", d, {"lds_rank": 8})
    assert all(n <= 2048 and 2 * u > n for n, u in paths["lds_rank"])  # mostly distinct keys


def test_outliers_lds_rank_path_thousands():
    d = depth_scene(40000, 35, "squeeze", zspread=0.2, outliers=True, culled=0.2, small=0.3)
    _, paths = _single("outliers 40k x0.2", d, {"lds_rank": 6})
    assert max(n for n, _ in paths["lds_rank"]) > 2048


def test_outliers_global_bitonic_and_lds_rank_in_one_frame():
    d = depth_scene(40000, 35, "squeeze", zspread=0.05, outliers=True, culled=0.2, small=0.3)
    _, paths = _single("outliers 40k x0.05", d, {"global_bitonic": 1, "lds_rank": 1})
    assert all(u > 1000 for _, u in paths["global_bitonic"])  # thousands of distinct keys, not a run of ties


def _levels_two_heavy():
    lv = np.linspace(-0.3, 0.3, 400).astype(np.float32).tolist()
    return lv + [0.0625] * 180 + [-0.1875] * 40


def test_levels_big_buckets_among_tiny_ones():
    """Two all-tied big buckets among some 400 tiny ones: k_bucket_rank's 64-key halo reaches into
    the big buckets' keys (which it must leave alone) on both sides."""
    d = depth_scene(12000, 36, "levels", levels=_levels_two_heavy())
    sizes, paths = _single("levels 400+2", d, {"lds_bitonic": 2})
    assert ((sizes > 0) & (sizes <= helpers.TINY_BUCKET)).sum() >= 300
    assert all(u <= 3 for _, u in paths["lds_bitonic"])


def test_above_512k_gaussians_unfused_sort():
    """P > 2^19: NB = 65536, so the bucket count runs on global atomics (k_bucket_count), the scan
    works on the slabs in global memory (the table does not fit its LDS staging) and the scatter is
    the unfused one -- with hundreds of large buckets behind them."""
    P = 540000
    assert helpers._nb(P) == 65536
    d = depth_scene(P, 37, "squeeze", zspread=1.0, outliers=True, culled=0.1, small=0.02)
    _single("540k", d, {"lds_rank": 300})


def test_synchronous_forward_frame_totals_launch(monkeypatch):
    """The synchronous gsr_forward (host read-back of R): k_frame_totals as a launch of its own ahead
    of the same sort."""
    from guava_renderer_amd.diff_gaussian_rasterization_32 import _C
    monkeypatch.setattr(_C, "ASYNC_BINNING_MB", 0)
    d = depth_scene(40000, 35, "squeeze", zspread=0.05, outliers=True, culled=0.2, small=0.3)
    _single("sync 40k x0.05", d, {"global_bitonic": 1, "lds_rank": 1})


# ---------------------------------------------------------------- batched

def _batch_gpu(sc, W, H, cams):
    """One BatchRasterizer forward: (colour, inverse depth, radii, decoded geometry arena)."""
    import torch
    from guava_renderer_amd.batch import BatchRasterizer
    B, P = len(cams), sc["means3D"].shape[0]
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    r = BatchRasterizer(B, P, W, H, R_capacity=40 * P * B, device="cuda")
    col, inv, radii = (x.cpu().numpy() for x in r.forward(*args, views, projs, tanf,
                                                          torch.zeros((B, 32), device="cuda")))
    assert not r.status()[1]
    lay = helpers.geom_layout(P, W, H, B)
    return col, inv, radii, helpers.decode(r.workspace[:helpers.layout_bytes(lay)].cpu().numpy(), lay)


def _batch(tag, sc, W, H, cams, need):
    """Frames of one cloud through the batched entry: images, radii and inverse depth per frame against
    the oracle bit-exactly, then the same sort checks on the workspace's geometry arena (which comes
    first in the workspace)."""
    import oracle
    B, P = len(cams), sc["means3D"].shape[0]
    col, inv, radii, gs = _batch_gpu(sc, W, H, cams)
    NB = helpers._nb(P)
    fstat = gs["ctrl"][helpers.CTRL_WORDS:].reshape(B, helpers.FS_WORDS)
    listed, got, frames = [], {}, []
    for f, c in enumerate(cams):
        o_col, o_radii, o_inv, os_ = oracle.forward(sc["means3D"], sc["colors"], sc["opacities"], sc["scales"],
                                                    sc["rotations"], None, c["viewmatrix"], c["projmatrix"], W, H,
                                                    c["tanfovx"], c["tanfovy"], np.zeros(32, np.float32))
        np.testing.assert_array_equal(radii[f], o_radii)
        np.testing.assert_array_equal(col[f], o_col)
        np.testing.assert_array_equal(inv[f], o_inv.reshape(H, W))
        sizes, paths = _check_frame(f"{tag} frame {f}", os_, gs["order"].reshape(B, P)[f],
                                    gs["bcount"].reshape(B, NB + 1)[f], gs["bstart"].reshape(B, NB + 1)[f],
                                    fstat[f], batched=True)
        listed += (f * NB + np.nonzero(sizes > helpers.TINY_BUCKET)[0]).tolist()
        frames.append(paths)
        for p, v in paths.items():
            got.setdefault(p, []).extend(v)
    assert int(gs["ctrl"][helpers.CTRL_NUM_BIG]) == len(listed), (tag, int(gs["ctrl"][helpers.CTRL_NUM_BIG]), len(listed))
    assert sorted(gs["big"][:len(listed)].tolist()) == listed, tag
    _assert_regime(tag, got, need)
    return frames


def _cams3(W, H):
    from guava_renderer_amd import camera
    return [camera.camera(W, H, distance=dist) for dist in (22.0, 20.0, 25.0)]


def test_batch_256_thread_rank_path():
    sc = depth_cloud(10000, 34, "squeeze", zspread=1.0, outliers=True, culled=0.2)
    _batch("batch outliers 10k", sc, 128, 96, _cams3(128, 96), {"256:lds_rank": 20})


def test_batch_256_thread_bitonic():
    lv = [-0.25, -0.125, -0.0625, 0.03125, 0.125, 0.25]
    sc = depth_cloud(12000, 38, "levels", levels=lv, culled=0.2)
    _batch("batch levels 6", sc, 64, 64, _cams3(64, 64), {"256:lds_bitonic": 18})


def test_batch_1024_thread_kernel():
    sc = depth_cloud(40000, 35, "squeeze", zspread=0.2, outliers=True, culled=0.2, small=0.3)
    # (the far frame's two end buckets are short enough for the 256-thread kernel)
    _batch("batch outliers 40k x0.2", sc, 64, 64, _cams3(64, 64), {"1024:lds_rank": 12, "256:lds_rank": 0})


def test_batch_global_bitonic():
    sc = depth_cloud(40000, 35, "squeeze", zspread=0.05, outliers=True, culled=0.2, small=0.3)
    frames = _batch("batch outliers 40k x0.05", sc, 64, 64, _cams3(64, 64),
                    {"1024:global_bitonic": 3, "1024:lds_rank": 1})
    assert all("1024:global_bitonic" in p for p in frames)


@pytest.mark.parametrize("P,path", [(2048, "256:lds_bitonic"), (2049, "1024:lds_bitonic")])
def test_batch_boundary_between_the_two_launches(P, path):
    """One tied bucket of exactly kSortSmallCap keys per frame is the 256-thread kernel's, one more
    key hands it to the 1024-thread kernel."""
    sc = depth_cloud(P, 39, "plane", small=0.3)
    frames = _batch(f"batch plane {P}", sc, 64, 64, _cams3(64, 64), {path: 3})
    assert all(p[path] == [(P, 1)] for p in frames)


def test_batch_worklist_from_one_frame_only():
    """Yaw spreads the tied levels over hundreds of small buckets: frame 1 lists nothing, so the
    batch worklist holds frame 0's buckets alone."""
    from guava_renderer_amd import camera
    lv = [-0.25, -0.125, -0.0625, 0.03125, 0.125, 0.25]
    sc = depth_cloud(12000, 38, "levels", levels=lv, culled=0.2)
    cams = [camera.camera(64, 64, yaw=0.0), camera.camera(64, 64, yaw=0.25)]
    frames = _batch("batch levels yaw", sc, 64, 64, cams, {"256:lds_bitonic": 6})
    assert len(frames[0]["256:lds_bitonic"]) == 6 and frames[1] == {}
