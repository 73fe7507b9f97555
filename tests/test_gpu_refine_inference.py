"""The refiner head on the inference paths (csrc/render_fwd.hip): forward-only batches
(`k_render_fwd_refine<., FWD = true>`), single frames on the quad-wave kernel
(`k_render_quad<., ., REFINE = true>`), the 16-byte fill of empty tiles under the head, and the fused
deform + head entry (gsr_forward_batch_deformed_refine).

Every comparison is torch.equal: nothing here has a tolerance and no pixel is left out.  The reference
of every case is the path that existed before: BatchRasterizer.forward(..., refine=head) without
forward_only at B = 3, computed once per (size, head, numerics) and never modified.  Before each call
under test out_color and head.out are filled with a sentinel NaN; afterwards out_color[:, keep:] must
still hold it and every element of head.out and out_color[:, :keep] must have been written.
gsr_render_variant (the launcher's own selection function) fails a case that misses its kernel.

The scene (B = 3, P = 4,000) asserts its preconditions from the reference forward's own tables:
  frame 0  a dense cloud of faint Gaussians: lists longer than one quad-ring refill (192 entries)
           whose pixels still take Gaussians past entry 192;
  frame 1  a camera that looks away: every tile empty (at B = 1: a frame with no work item but empties);
  frame 2  ~200 opaque Gaussians stacked over a quarter of the image and ~50 tiny ones: pixels that
           stop early, strips without a survivor inside non-empty tiles, empty tiles.
Sizes: 64x48 (tile-aligned, 16-byte-aligned outputs: the fill), 50x37 (W % 4 != 0, partial tiles on
both axes), 64x48 with out_color and out_refine one float into their buffers (the fill's fallback).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 32
P = 4000
SENT = 0x7FC12345  # a NaN no kernel writes (the overflow fill's is 0x7FC00000)
SIZES = {"aligned": (64, 48, 0), "ragged": (50, 37, 0), "offset": (64, 48, 1)}
# (n_out, keep, bias, backgrounds): the head shapes of the refine tests, each bias / background kind twice
HEADS = [(16, 4, True, "per_frame"), (3, 0, False, "one"), (28, 4, True, "one"), (1, 31, False, "per_frame"),
         (16, 4, False, "one")]
HEAD_IDS = ["16+4-bias-bgB", "3+0-nobias-bg1", "28+4-bias-bg1", "1+31-nobias-bgB", "16+4-nobias-bg1"]
ATTRS = ("means3D", "colors", "opacities", "scales", "rotations")


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def _nm(name, forward_only=False):
    from guava_renderer_amd import _lib
    return _lib.numerics(fast_exp=name == "fast_exp") | (_lib.FORWARD_ONLY if forward_only else 0)


@functools.lru_cache(maxsize=None)
def _scene(W, H):
    """[means3D [3,P,3], colors [P,32], opacities, scales, rotations [3,P,k], views, projs, tanfov]."""
    from guava_renderer_amd import camera, scenes
    rng = np.random.default_rng(21)
    sc = scenes.random_cloud(P, seed=6)
    per = {k: np.repeat(sc[k][None], 3, 0).copy() for k in ("means3D", "opacities", "scales", "rotations")}
    # frame 0: faint, so no pixel runs out of transmittance and the lists are walked to their ends
    per["opacities"][0] = np.maximum(0.06 * sc["opacities"], np.float32(0.02))
    # frame 2 (the camera sees x in +-0.92, y in -0.6 +- 0.92: tanfov 1/24 at distance 22)
    n_big, n_small = 200, 50
    m = np.empty((P, 3), np.float32)
    m[:] = (0.0, 0.0, -100.0)  # the rest: behind the camera, culled
    m[:n_big, 0] = -0.45 + rng.uniform(-0.03, 0.03, n_big)
    m[:n_big, 1] = -0.95 + rng.uniform(-0.03, 0.03, n_big)
    m[:n_big, 2] = np.linspace(-0.3, 0.3, n_big)
    m[n_big:n_big + n_small, 0] = rng.uniform(0.1, 0.85, n_small)
    m[n_big:n_big + n_small, 1] = rng.uniform(-1.25, 0.05, n_small)
    m[n_big:n_big + n_small, 2] = rng.uniform(-0.3, 0.3, n_small)
    s = np.full((P, 3), 0.004, np.float32)
    s[:n_big] = 0.12
    per["means3D"][2], per["scales"][2] = m, s
    per["opacities"][2] = 0.99
    cams = [camera.camera(W, H), camera.camera(W, H, distance=-22.0), camera.camera(W, H)]
    views = _t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = _t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = _t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    return (_t(per["means3D"]), _t(sc["colors"]), _t(per["opacities"]), _t(per["scales"]), _t(per["rotations"]),
            views, projs, tanf)


@functools.lru_cache(maxsize=None)
def _bg(kind):
    bg = np.random.default_rng(22).uniform(-1.0, 1.0, (3, C)).astype(np.float32)
    return _t(bg) if kind == "per_frame" else _t(bg[0])


def _args(size, cfg, frame=None):
    """forward()'s positional arguments: the whole batch, or frame `frame` alone (B = 1)."""
    W, H, _ = SIZES[size]
    a = list(_scene(W, H))
    bg = _bg(cfg[3])
    if frame is None:
        return a + [bg]
    k = frame
    one = [a[0][k:k + 1], a[1], a[2][k:k + 1], a[3][k:k + 1], a[4][k:k + 1], a[5][k:k + 1], a[6][k:k + 1],
           a[7][k:k + 1]]
    return one + [bg[k:k + 1] if bg.dim() == 2 else bg]


def _head(cfg, seed=5):
    from guava_renderer_amd.batch import RefineHead
    n_out, keep, bias, _ = cfg
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.3, (n_out, C)).astype(np.float32)
    b = rng.normal(0, 0.5, (n_out,)).astype(np.float32)
    return RefineHead(_t(w), _t(b) if bias else None, negative_slope=0.2, keep_channels=keep)


def _offset_view(shape, offset):
    n = int(np.prod(shape))
    store = torch.empty((n + 4,), dtype=torch.float32, device=DEV)
    assert store.data_ptr() % 16 == 0
    v = store[offset:offset + n].view(*shape)
    assert v.data_ptr() % 16 == 4 * offset
    return v


def _rig(B, size, cfg, R_capacity=None, head=None):
    """(rasterizer, head) with the size's output placement: `offset` puts out_color and head.out one
    float into their buffers."""
    from guava_renderer_amd.batch import BatchRasterizer
    W, H, offset = SIZES[size]
    r = BatchRasterizer(B, P, W, H, R_capacity=R_capacity or 64 * P * B, device=DEV)
    head = head or _head(cfg)
    if offset:
        r.out_color = _offset_view((B, C, H, W), offset)
    # the head's output of this stream and shape (RefineHead.epilogue), placed here so that it can be
    # filled before the call and sit off 16-byte alignment
    key = (torch.cuda.current_stream(DEV).cuda_stream, (B, head.n_out, H, W))
    head._outs[key] = _offset_view((B, head.n_out, H, W), offset)
    head.out = head._outs[key]
    return r, head


def _fill(r, head):
    for x in (r.out_color, head.out, r.out_invdepth):
        x.view(torch.int32).fill_(SENT)
    r.radii.fill_(-7)


def _run(r, head, call):
    """Sentinel-fill, run `call()` (a forward on r with refine=head), check what was and was not
    written, and return the outputs as clones."""
    keep = head.keep_channels
    _fill(r, head)
    col, inv, radii = call()
    torch.cuda.synchronize()
    R, ovf = r.status()
    assert not ovf
    assert col.data_ptr() == r.out_color.data_ptr()
    ci, oi = r.out_color.view(torch.int32), head.out.view(torch.int32)
    assert (ci[:, keep:] == SENT).all(), "out_color channels from keep on were written"
    assert not (ci[:, :keep] == SENT).any() and not (oi == SENT).any() and \
        not (inv.view(torch.int32) == SENT).any(), "an output element was not written"
    return dict(raw=col[:, :keep].clone(), refined=head.out.clone(), inv=inv.clone(), radii=radii.clone(), R=R)


def _same(ref, got, frames=slice(None), what=""):
    for k in ("raw", "refined", "inv", "radii"):
        assert torch.equal(ref[k][frames], got[k]), (what, k)


def _rows(r):
    """final_T, n_contrib [B,H,W], list length per tile [B*T], strip_cnt [B*T,4] of the last forward."""
    B, W, H = r.B, r.W, r.H
    T = ((W + 15) // 16) * ((H + 15) // 16)
    _, st, _ = helpers.decode_batch_workspace(r, geom=False)
    rg = st["ranges"].reshape(B * T, 2).astype(np.int64)
    return (st["final_T"].reshape(B, H, W), st["n_contrib"].reshape(B, H, W), rg[:, 1] - rg[:, 0],
            st["strip_cnt"].reshape(B * T, 4))


@functools.lru_cache(maxsize=None)
def _reference(size, ci, numerics):
    """The existing path: forward(refine=head) at B = 3, not forward-only.  Asserts the scene's
    preconditions from this forward's tables; returns (outputs, final_T, n_contrib, empty-tile mask)."""
    from guava_renderer_amd import _lib
    cfg = HEADS[ci]
    W, H, _ = SIZES[size]
    assert _lib.render_variant(3, _nm(numerics), True) == "refine"
    r, head = _rig(3, size, cfg)
    out = _run(r, head, lambda: r.forward(*_args(size, cfg), refine=head, numerics=_nm(numerics)))
    final_T, n_contrib, n_list, strip_cnt = _rows(r)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    inside = np.array([(t % gx + 1) * 16 <= W and (t // gx + 1) * 16 <= H for t in range(T)] * 3)
    # empty tiles wholly inside the image (frame 1 is nothing else), and in frame 2 beside non-empty ones
    assert not n_list[T:2 * T].any() and ((n_list == 0) & inside).any()
    assert (n_list[:T] > 0).all() and (n_list[2 * T:] > 0).any() and (n_list[2 * T:] == 0).any()
    # strips without a survivor inside non-empty tiles
    assert ((strip_cnt == 0) & (n_list[:, None] > 0)).any()
    # early-terminated pixels: transmittance used up (T < 0.01: the next opaque Gaussian would pass
    # the 1e-4 stop) more than a chunk before the end of a list of opaque Gaussians that cover them
    tile_of = (np.arange(H)[:, None] // 16) * gx + np.arange(W)[None, :] // 16
    n2 = n_list[2 * T:][tile_of]
    assert ((final_T[2] < 0.01) & (n_contrib[2] + 64 < n2)).sum() >= 16
    # dense frame: a list longer than one quad-ring refill, walked past its 192nd entry
    assert n_list[:T].max() > 192 and (n_contrib[0] > 192).sum() >= 16
    empty_px = torch.from_numpy((n_list.reshape(3, T)[:, tile_of] == 0))  # [3,H,W]
    assert (out["refined"].isfinite()).all() and (out["refined"] < 0).any() and (out["refined"] > 0).any()
    return out, torch.from_numpy(final_T.copy()), torch.from_numpy(n_contrib.astype(np.int64)), empty_px


# ----------------------------------------------------------------------------- 1. forward-only batch

@pytest.mark.parametrize("numerics", ["exact", "fast_exp"])
@pytest.mark.parametrize("ci", range(len(HEADS)), ids=HEAD_IDS)
@pytest.mark.parametrize("size", list(SIZES))
def test_forward_only_batch_equals_the_full_refine_forward(size, ci, numerics):
    from guava_renderer_amd import _lib
    cfg = HEADS[ci]
    ref = _reference(size, ci, numerics)[0]
    assert _lib.render_variant(3, _nm(numerics, True), True) == "refine_fwd"
    r, head = _rig(3, size, cfg)
    got = _run(r, head, lambda: r.forward(*_args(size, cfg), refine=head, numerics=_nm(numerics),
                                          forward_only=True))
    _same(ref, got)
    assert got["R"] == ref["R"]


@pytest.mark.parametrize("numerics", ["exact", "fast_exp"])
@pytest.mark.parametrize("size", ["aligned", "ragged"])
def test_forward_only_leaves_the_backward_rows_to_the_next_full_forward(size, numerics):
    """final_T / n_contrib poisoned, a forward-only refine call (which stores neither and whose
    backward is refused), then a full refine forward + backward_refine: both rows come back bit for
    bit as the reference forward left them."""
    from guava_renderer_amd._lib import GsrError
    ci = 0
    cfg = HEADS[ci]
    W, H, _ = SIZES[size]
    ref, T_ref, n_ref, _ = _reference(size, ci, numerics)
    r, head = _rig(3, size, cfg)
    args = _args(size, cfg)
    n4 = 4 * 3 * H * W
    off_T = helpers.layout_bytes(helpers.geom_layout(P, W, H, 3))
    off_n = off_T + helpers._align(n4)
    r.workspace[off_T:off_T + n4].fill_(0xFF)
    r.workspace[off_n:off_n + n4].fill_(0xFF)
    got = _run(r, head, lambda: r.forward(*args, refine=head, numerics=_nm(numerics), forward_only=True))
    _same(ref, got)
    for o in (off_T, off_n):  # the forward-only kernel stores neither row
        assert (r.workspace[o:o + n4] == 0xFF).all()
    rng = np.random.default_rng(3)
    dref = _t(rng.normal(size=tuple(head.out.shape)).astype(np.float32))
    with pytest.raises(GsrError):
        r.backward_refine(head, *args, dref, numerics=_nm(numerics))
    full = _run(r, head, lambda: r.forward(*args, refine=head, numerics=_nm(numerics)))
    _same(ref, full)
    g = r.backward_refine(head, *args, dref, numerics=_nm(numerics))
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in g.values() if v is not None) and g["weight"].abs().max() > 0
    final_T, n_contrib, _, _ = _rows(r)
    assert torch.equal(torch.from_numpy(final_T.copy()).view(torch.int32), T_ref.view(torch.int32))
    assert torch.equal(torch.from_numpy(n_contrib.astype(np.int64)), n_ref)


# ----------------------------------------------------------------------------- 2. the fill under the head

@pytest.mark.parametrize("numerics", ["exact", "fast_exp"])
@pytest.mark.parametrize("ci", range(len(HEADS)), ids=HEAD_IDS)
def test_refine_fill_equals_the_strip_stores(ci, numerics):
    """The differentiable refine kernel at 64x48: 16-byte-aligned outputs take the fill for empty tiles,
    outputs one float off take store_strip -- same images, and the empty tiles' final_T / n_contrib
    are 1 / 0 either way."""
    a, Ta, na, empty = _reference("aligned", ci, numerics)
    b, Tb, nb, _ = _reference("offset", ci, numerics)
    _same(a, b)
    assert a["R"] == b["R"]
    assert empty.any() and (Ta[empty] == 1.0).all() and (na[empty] == 0).all()
    assert torch.equal(Ta.view(torch.int32), Tb.view(torch.int32)) and torch.equal(na, nb)
    # an empty tile's pixels hold one value per channel (the head applied to the frame's background)
    assert empty[1].all() and empty[2].any() and not empty[0].any()
    for f in (1, 2):
        px = a["refined"][f][:, empty[f].to(DEV)]  # [n_out, pixels]
        assert (px == px[:, :1]).all()


# ----------------------------------------------------------------------------- 3. one frame: quad waves

@pytest.mark.parametrize("numerics", ["exact", "fast_exp"])
@pytest.mark.parametrize("ci", range(len(HEADS)), ids=HEAD_IDS)
@pytest.mark.parametrize("size", list(SIZES))
def test_single_frame_quad_waves_equal_the_batch_frames(size, ci, numerics):
    """Frame k alone (B = 1: the quad-wave kernel with the head's epilogue) equals frame k of the
    B = 3 reference, differentiable and forward-only: the dense frame (several ring refills), the
    all-empty frame and the sparse one."""
    from guava_renderer_amd import _lib
    cfg = HEADS[ci]
    ref = _reference(size, ci, numerics)[0]
    assert _lib.render_variant(1, _nm(numerics), True) == "quad_refine"
    assert _lib.render_variant(1, _nm(numerics, True), True) == "quad_refine"
    r, head = _rig(1, size, cfg)
    R_sum = {False: 0, True: 0}
    for k in range(3):
        args = _args(size, cfg, frame=k)
        for fo in (False, True):
            got = _run(r, head, lambda: r.forward(*args, refine=head, numerics=_nm(numerics), forward_only=fo))
            _same(ref, got, slice(k, k + 1), f"frame {k} forward_only={fo}")
            R_sum[fo] += got["R"]
    assert R_sum[False] == ref["R"] and R_sum[True] == ref["R"]


# ----------------------------------------------------------------------------- 4. fused deform + head

@functools.lru_cache(maxsize=None)
def _avatar():
    """The test avatar on the SMPL-X template fixture: assets, EHM parameters of 3 frames, cameras."""
    from guava_renderer_amd import avatar, scenes
    body, flame, extra = avatar.ehm_assets(seed=0)
    verts, faces, tex = avatar.template_mesh()
    g = avatar.gaussians(verts, faces, tex, P=12000, seed=0)
    bp, fp = avatar.ehm_params(3, seed=3000)
    cams = scenes.frame_cameras(3, 96, 96, seed=7)
    views = _t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = _t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = _t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    bg = _t(np.random.default_rng(23).uniform(-1.0, 1.0, (3, C)).astype(np.float32))
    return body, flame, extra, g, bp, fp, (views, projs, tanf), bg


def _pipe(B, frames, R_capacity=None):
    from guava_renderer_amd.pipeline import AvatarPipeline
    body, flame, extra, g, bp, fp, cams, bg = _avatar()
    pipe = AvatarPipeline(body, flame, extra, g, B, 96, 96, R_capacity=R_capacity or 48 * 12000 * B, device=DEV)
    pipe.bg = bg[frames].contiguous()
    params = ({k: _t(v[frames]) for k, v in bp.items()}, {k: _t(v[frames]) for k, v in fp.items()})
    return pipe, params, tuple(c[frames] for c in cams)


def _avatar_rig(pipe, cfg):
    """The pipeline's rasterizer with a head whose output can be sentinel-filled."""
    head = _head(cfg)
    key = (torch.cuda.current_stream(DEV).cuda_stream, (pipe.B, head.n_out, 96, 96))
    head._outs[key] = torch.empty(key[1], dtype=torch.float32, device=DEV)
    head.out = head._outs[key]
    return head


@pytest.mark.parametrize("ci", [0, 3], ids=[HEAD_IDS[0], HEAD_IDS[3]])
def test_fused_deform_with_the_head_equals_the_two_step_path(ci):
    """96x96 avatar, B = 3 and B = 1: forward_deformed(refine=head) equals deformer.forward() +
    forward(refine=head) (the reference: B = 3, not forward-only), and AvatarPipeline.render(fused=True,
    refine=head) equals fused=False."""
    from guava_renderer_amd import _lib
    cfg = HEADS[ci]
    pipe, params, cams = _pipe(3, slice(0, 3))
    r, head = pipe.rast, _avatar_rig(pipe, cfg)
    e = pipe.ehm(*params)
    verts, vt = e["vertices"], e["ver_transform_mat"]
    d = pipe.gauss(verts, vt)
    ref = _run(r, head, lambda: r.forward(d["xyz"], pipe.gauss.colors, pipe.gauss.opacity, d["scaling"],
                                          d["rotation"], *cams, pipe.bg, refine=head))
    assert (ref["radii"] > 0).sum() > pipe.P and not pipe.gauss.bad_index()
    assert _lib.render_variant(3, _lib.FORWARD_ONLY, True) == "refine_fwd"
    got = _run(r, head, lambda: r.forward_deformed(pipe.gauss, verts, vt, *cams, pipe.bg, refine=head))
    _same(ref, got, what="forward_deformed B=3")
    assert got["R"] == ref["R"]
    two = _run(r, head, lambda: pipe.render(*params, *cams, refine=head)[:3])
    fused = _run(r, head, lambda: pipe.render(*params, *cams, refine=head, fused=True)[:3])
    _same(ref, two, what="render B=3")
    _same(two, fused, what="render fused B=3")
    assert pipe.render(*params, *cams, refine=head, fused=True)[3] is None
    # B = 1: frame k of the same EHM output through the fused entry (quad waves with the head)
    pipe1, params1, cams1 = _pipe(1, slice(1, 2))
    r1, head1 = pipe1.rast, _avatar_rig(pipe1, cfg)
    got1 = _run(r1, head1, lambda: r1.forward_deformed(pipe1.gauss, verts[1:2], vt[1:2], *cams1, pipe1.bg,
                                                       refine=head1))
    _same(ref, got1, slice(1, 2), "forward_deformed B=1")
    two1 = _run(r1, head1, lambda: pipe1.render(*params1, *cams1, refine=head1)[:3])
    fused1 = _run(r1, head1, lambda: pipe1.render(*params1, *cams1, refine=head1, fused=True)[:3])
    _same(two1, fused1, what="render fused B=1")


def test_fused_deform_with_the_head_flags_a_bad_binding_face():
    """An out-of-range binding face still sets bad_index_flag (and drops that Gaussian) with the head."""
    cfg = HEADS[0]
    pipe, params, cams = _pipe(3, slice(0, 3))
    head = _avatar_rig(pipe, cfg)
    e = pipe.ehm(*params)
    n_faces = pipe.gauss.faces.shape[0]
    pipe.gauss.bind[17] = n_faces + 3
    assert not pipe.gauss.bad_index()
    got = _run(pipe.rast, head, lambda: pipe.rast.forward_deformed(pipe.gauss, e["vertices"], e["ver_transform_mat"],
                                                                   *cams, pipe.bg, refine=head))
    assert pipe.gauss.bad_index()
    assert got["radii"][:, pipe.gauss.V + 17].eq(0).all() and (got["radii"] > 0).sum() > pipe.P


# ----------------------------------------------------------------------------- 5. capacity overflow

def _assert_overflow(r, head, call):
    from guava_renderer_amd._lib import CapacityError
    _fill(r, head)
    call()
    torch.cuda.synchronize()
    assert r.status()[1] and int(r.overflow_flag().item()) == 1
    for x in (r.out_color, r.out_invdepth, head.out):
        assert torch.isnan(x).all() and not (x.view(torch.int32) == SENT).any()
    with pytest.raises(CapacityError):
        r.poll(wait=True)


@pytest.mark.parametrize("B", [3, 1])
def test_overflow_fills_nan_on_the_batch_paths(B):
    """R_capacity too small: the forward-only refine batch (B = 3) and the quad-refine frame (B = 1)
    render NaN into out_color, the inverse depth and head.out, and the next poll raises."""
    cfg = HEADS[0]
    r, head = _rig(B, "aligned", cfg, R_capacity=500)
    args = _args("aligned", cfg) if B == 3 else _args("aligned", cfg, frame=0)
    _assert_overflow(r, head, lambda: r.forward(*args, refine=head, forward_only=True))
    if B == 1:
        _assert_overflow(r, head, lambda: r.forward(*args, refine=head))


@pytest.mark.parametrize("B", [3, 1])
def test_overflow_fills_nan_on_the_fused_deform_path(B):
    pipe, params, cams = _pipe(B, slice(0, B), R_capacity=500)
    head = _avatar_rig(pipe, HEADS[0])
    _assert_overflow(pipe.rast, head, lambda: pipe.render(*params, *cams, refine=head, fused=True))


# ----------------------------------------------------------------------------- 6. argument checks

@pytest.mark.parametrize("bad", ["n_out_zero", "too_many_channels", "null_out_refine"])
def test_deformed_refine_rejects_a_bad_epilogue(bad):
    """gsr_forward_batch_deformed_refine checks the epilogue as gsr_forward_batch_refine does:
    GSR_ERR_ARG (1) for n_out = 0, keep + n_out > 32 or a NULL out_refine; nothing is launched."""
    from guava_renderer_amd import _lib
    from guava_renderer_amd.batch import RefineHead

    class BadHead(RefineHead):
        def epilogue(self, B, H, W):
            ep = super().epilogue(B, H, W)
            if bad == "n_out_zero":
                ep.n_out = 0
            elif bad == "too_many_channels":
                ep.keep_channels = C - self.n_out + 1
            else:
                ep.out_refine = None
            return ep

    pipe, params, cams = _pipe(3, slice(0, 3))
    good = _head(HEADS[0])
    head = BadHead(good.weight, good.bias, 0.2, good.keep_channels)
    e = pipe.ehm(*params)
    pipe.rast.out_color.view(torch.int32).fill_(SENT)
    with pytest.raises(_lib.GsrError, match=r"gsr_forward_batch_deformed_refine failed \(1\)"):
        pipe.rast.forward_deformed(pipe.gauss, e["vertices"], e["ver_transform_mat"], *cams, pipe.bg, refine=head)
    torch.cuda.synchronize()
    assert (pipe.rast.out_color.view(torch.int32) == SENT).all()
    # the raw entry point with a NULL deform block is still refused before anything else
    ep = good.epilogue(3, 96, 96)
    rc = _lib.load().gsr_forward_batch_deformed_refine(3, 96, 96, None, None, 0, None, 0, 1.0, None, None, None,
                                                        None, 0, None, 0, None, None, None, 0, ctypes.byref(ep), 0,
                                                        None)
    assert rc == -1
