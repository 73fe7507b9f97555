"""The forward-only instantiation of the batched compositing kernel (csrc/render_fwd.hip, FWD).

A batched forward with GSR_FORWARD_ONLY (BatchRasterizer.forward(forward_only=True), the call
AvatarPipeline.render and the bench make) runs `k_render_fwd<..., FWD = true>`: no last-contributor
tracking, no final_T / n_contrib stores.  Its colour, inverse depth, radii and instance count must
equal the full forward's bit for bit (torch.equal) on the same inputs; nothing here has a tolerance.
The batched strip kernel runs from B = 2, the smallest batch used.

Reference of every test: the full forward of the same BatchRasterizer call, computed once per case
(lru_cache) and never modified.
"""
import functools

import numpy as np
import pytest
import torch

import deform_cases
import helpers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 32


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def _cam_args(cams):
    views = _t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = _t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = _t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    return [views, projs, tanf]


ATTRS = ("means3D", "colors", "opacities", "scales", "rotations")


@functools.lru_cache(maxsize=None)
def _cloud_args(W, H):
    """The shared avatar cloud under two cameras: [attributes..., views, projs, tanfov]."""
    from guava_renderer_amd import camera, scenes
    sc = scenes.avatar_cloud(6000, seed=4)
    cams = [camera.camera(W, H, yaw=y, pitch=-0.3 * y) for y in (0.0, 0.5)]
    return tuple([_t(sc[k]) for k in ATTRS] + _cam_args(cams))


@functools.lru_cache(maxsize=None)
def _backgrounds(B, kind):
    if kind == "zeros":
        return torch.zeros((B, C), device=DEV)
    return _t(np.random.default_rng(11).uniform(0.0, 1.0, (B, C)).astype(np.float32))


def _numerics(name):
    from guava_renderer_amd import _lib
    return {"exact": 0, "split_bf16": _lib.numerics(split_bf16=True), "fast_exp": _lib.numerics(fast_exp=True)}[name]


def _poison(r):
    """Fill the outputs so that a pixel the next forward does not write cannot pass for one it wrote."""
    for x in r.out_color, r.out_invdepth:
        x.fill_(7.0)
    r.radii.fill_(-7)


def _full_then_forward_only(r, args, **kw):
    """(full forward's outputs and instance count, forward-only's) on the same rasterizer and inputs."""
    _poison(r)
    ref = [x.clone() for x in r.forward(*args, **kw)]
    torch.cuda.synchronize()
    R_ref, ovf = r.status()
    assert not ovf and R_ref > 0
    _poison(r)
    got = [x.clone() for x in r.forward(*args, forward_only=True, **kw)]
    torch.cuda.synchronize()
    return ref, R_ref, got, r.status()[0]


def _assert_same(ref, R_ref, got, R_got):
    assert R_got == R_ref
    for name, a, b in zip(("color", "invdepth", "radii"), ref, got):
        assert torch.equal(a, b), name
    assert not torch.isnan(ref[0]).any() and not (ref[0] == 7.0).all()


# ----------------------------------------------------------------------------- 1. numerics x background

@pytest.mark.parametrize("bg", ["zeros", "random"])
@pytest.mark.parametrize("numerics", ["exact", "split_bf16", "fast_exp"])
def test_parity_across_numerics_and_backgrounds(numerics, bg):
    """B = 2, 160x128 (tile-aligned: empty tiles take the 16-byte fill).  The cloud's features are one
    table for both frames, so split_bf16 runs the pre-split instantiation (SPLIT = 2), exact and
    fast_exp the f32 one, in both EXACT values."""
    from guava_renderer_amd.batch import BatchRasterizer
    B, W, H = 2, 160, 128
    args = list(_cloud_args(W, H)) + [_backgrounds(B, bg)]
    r = BatchRasterizer(B, 6000, W, H, R_capacity=40 * 6000 * B, device=DEV)
    ref, R_ref, got, R_got = _full_then_forward_only(r, args, numerics=_numerics(numerics))
    _assert_same(ref, R_ref, got, R_got)
    if bg == "random":  # the background reaches the image: an empty corner pixel is exactly bg
        assert torch.equal(got[0][:, :, 0, 0], args[-1])


# ----------------------------------------------------------------------------- 2. ragged image

@pytest.mark.parametrize("W,H,offset", [(150, 100, 0), (150, 100, 1), (160, 128, 1)])
def test_ragged_image_and_unaligned_output(W, H, offset):
    """150x100: partial strips on both edges, and no tile passes the 16-byte fill's conditions, so
    empty tiles are stored strip by strip.  offset = 1: out_color is a view one float into its
    buffer, which fails the fill's alignment test (at 160x128 that alone decides the path)."""
    from guava_renderer_amd.batch import BatchRasterizer
    B = 2
    args = list(_cloud_args(W, H)) + [_backgrounds(B, "random")]
    r = BatchRasterizer(B, 6000, W, H, R_capacity=40 * 6000 * B, device=DEV)
    if offset:
        n = B * C * H * W
        store = torch.empty((n + 4,), dtype=torch.float32, device=DEV)
        assert store.data_ptr() % 16 == 0
        r.out_color = store[offset:offset + n].view(B, C, H, W)
        assert r.out_color.data_ptr() % 16 == 4 * offset
    ref, R_ref, got, R_got = _full_then_forward_only(r, args)
    _assert_same(ref, R_ref, got, R_got)
    assert (ref[0] != 7.0).all()  # every pixel of the ragged image was written


# ----------------------------------------------------------------------------- 3. every epilogue path

def _batch_image_state(r):
    """final_T, n_contrib [B,H,W], ranges [B*T,2] and strip_cnt [B*T,4] of the last (full) forward:
    the head of the batch workspace's image arena (carve_image in csrc/capi.hip)."""
    B, W, H = r.B, r.W, r.H
    T = ((W + 15) // 16) * ((H + 15) // 16)
    _, st, _ = helpers.decode_batch_workspace(r, geom=False)
    return (st["final_T"].reshape(B, H, W), st["n_contrib"].reshape(B, H, W), st["ranges"].reshape(B * T, 2),
            st["strip_cnt"].reshape(B * T, 4))


def test_every_epilogue_path_in_one_launch():
    """B = 3: a frame that sees the cloud, a frame whose camera looks away (every tile empty), and a
    frame of ~200 large opaque Gaussians stacked in depth over a quarter of the image plus ~50 tiny
    ones elsewhere: whole strips that stop early (every pixel done), strips without a survivor inside
    non-empty tiles, and empty tiles -- each asserted from the full forward's workspace."""
    from guava_renderer_amd import camera, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    B, P, W, H = 3, 6000, 160, 128
    rng = np.random.default_rng(8)
    sc = scenes.avatar_cloud(P, seed=4)
    per = {k: np.repeat(sc[k][None], B, 0).copy() for k in ("means3D", "opacities", "scales", "rotations")}
    # frame 2: the camera sees x in +-0.92, y in -0.6 +- 0.92 (tanfov 1/24 at distance 22)
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
    args = [_t(per["means3D"]), _t(sc["colors"]), _t(per["opacities"]), _t(per["scales"]), _t(per["rotations"])]
    args += _cam_args(cams) + [_backgrounds(B, "random")]
    r = BatchRasterizer(B, P, W, H, R_capacity=40 * P * B, device=DEV)
    _poison(r)
    ref = [x.clone() for x in r.forward(*args)]
    torch.cuda.synchronize()
    R_ref, ovf = r.status()
    assert not ovf
    final_T, n_contrib, ranges, strip_cnt = _batch_image_state(r)
    gx, T = (W + 15) // 16, ((W + 15) // 16) * ((H + 15) // 16)
    n_list = (ranges[:, 1] - ranges[:, 0]).astype(np.int64)
    # frame 0 renders, frame 1 is all empty tiles, frame 2 has empty and non-empty tiles
    assert (n_list[:T] > 0).sum() > 4 and (ref[2][0] > 0).sum() > 1000
    assert not n_list[T:2 * T].any() and not (ref[2][1] > 0).any()
    assert (n_list[2 * T:] == 0).any() and (n_list[2 * T:] > 0).any()
    assert torch.equal(ref[0][1], args[-1][1][:, None, None].expand(C, H, W))
    # strips with no survivor inside non-empty tiles (the strip_cnt == 0 shortcut), in frame 2
    assert ((strip_cnt[2 * T:] == 0) & (n_list[2 * T:, None] > 0)).any()
    # whole strips that stopped early in frame 2: every pixel of the 8x8 strip ended far before the
    # end of its tile's list (more than one 64-entry chunk left) with its transmittance used up --
    # only a pixel that is done stops taking opaque Gaussians that cover it
    early = 0
    for t in np.flatnonzero(n_list[2 * T:] >= 150):
        tx, ty = t % gx, t // gx
        for sy in range(2):
            for sx in range(2):
                y0, x0 = ty * 16 + 8 * sy, tx * 16 + 8 * sx
                nc, ft = n_contrib[2, y0:y0 + 8, x0:x0 + 8], final_T[2, y0:y0 + 8, x0:x0 + 8]
                if nc.shape == (8, 8) and (nc < n_list[2 * T + t] - 64).all() and (ft < 0.01).all():
                    early += 1
    assert early >= 4, early
    _poison(r)
    got = [x.clone() for x in r.forward(*args, forward_only=True)]
    torch.cuda.synchronize()
    _assert_same(ref, R_ref, got, r.status()[0])


# ----------------------------------------------------------------------------- 4. workspace hygiene

def _two_strip_args(B, P, W, H):
    """A scene whose backward is bit-reproducible.  render_bwd sums a Gaussian's gradient over the
    strips it reaches with float atomics, so gradients of an arbitrary scene differ in their last bits
    from run to run (test_gpu_deform_backward.py compares them at a scale bar for that reason).  A
    float sum of at most two terms does not depend on their order: here every Gaussian is small
    (alpha >= 1/255 within 2.7 pixels of its centre) and centred 3.5 to 4.5 pixels into its 8-pixel
    strip column, so it reaches one strip, or two across a horizontal strip edge, never more.  Both
    frames share the camera (the placement is in pixels); opacities are per frame."""
    from guava_renderer_amd import camera
    rng = np.random.default_rng(13)
    cam = camera.camera(W, H)
    tanf = cam["tanfovx"]
    xp = 8.0 * rng.integers(0, W // 8, P) + rng.uniform(3.5, 4.5, P)
    yp = rng.uniform(0.0, H - 1.0, P)
    zv = 22.0 + rng.uniform(-0.05, 0.05, P)  # view-space depth (camera.look_at_w2c: R = I, t = (0, 0.6, 22))
    m = np.stack([((2 * xp + 1) / W - 1) * zv * tanf, ((2 * yp + 1) / H - 1) * zv * tanf - 0.6, zv - 22.0], 1)
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    attrs = [_t(m.astype(np.float32)), _t(rng.uniform(0.0, 1.0, (P, C)).astype(np.float32)),
             _t(rng.uniform(0.3, 0.95, (B, P, 1)).astype(np.float32)),
             _t(np.full((P, 3), 0.0065, np.float32)), _t(q.astype(np.float32))]
    return attrs + _cam_args([cam] * B) + [_backgrounds(B, "random")]


def test_full_forward_after_forward_only_gives_the_same_gradients():
    """full forward + backward, forward-only (its backward is refused), full forward + backward: the
    second gradients equal the first bit for bit -- the forward-only kernel leaves nothing behind
    that a later full forward does not rewrite.  Between the two, the final_T and n_contrib rows are
    poisoned.  On the avatar cloud the two rows themselves are compared (they are all the backward
    reads of what the forward-only kernel no longer writes); the gradients are compared on a scene
    whose backward is reproducible to the bit (_two_strip_args)."""
    from guava_renderer_amd._lib import GsrError
    from guava_renderer_amd.batch import BatchRasterizer
    B, P, W, H = 2, 6000, 160, 128
    rng = np.random.default_rng(12)
    dL = _t(rng.normal(size=(B, C, H, W)).astype(np.float32))
    dLi = _t(rng.normal(size=(B, H, W)).astype(np.float32))
    r = BatchRasterizer(B, P, W, H, R_capacity=40 * P * B, device=DEV)
    # the two rows head the image arena, each 256-byte aligned (carve_image in csrc/capi.hip)
    n4 = 4 * B * H * W
    off_T = helpers.layout_bytes(helpers.geom_layout(P, W, H, B))
    off_n = off_T + helpers._align(n4)

    def full(args):
        out = [x.clone() for x in r.forward(*args)]
        g = r.backward(*args, dL, dLi)
        torch.cuda.synchronize()
        rows = [r.workspace[o:o + n4].clone() for o in (off_T, off_n)]
        return out, rows, {k: v.clone() for k, v in g.items() if v is not None}

    for name, args in (("cloud", list(_cloud_args(W, H)) + [_backgrounds(B, "random")]),
                       ("two_strip", _two_strip_args(B, P, W, H))):
        out0, rows0, g0 = full(args)
        assert all(torch.isfinite(v).all() for v in g0.values()) and g0["colors"].abs().max() > 0
        T0 = rows0[0].view(torch.float32)
        assert (T0 < 0.5).sum() > 500 and (rows0[1].view(torch.int32) > 1).sum() > 500  # a real render
        r.workspace[off_T:off_n + n4].fill_(0xFF)  # final_T = NaN, n_contrib = 0xFFFFFFFF
        _poison(r)
        r.forward(*args[:-1], _backgrounds(B, "zeros"), forward_only=True)
        with pytest.raises(GsrError):
            r.backward(*args, dL, dLi)
        out1, rows1, g1 = full(args)
        for a, b in zip(out0 + rows0, out1 + rows1):
            assert torch.equal(a, b), name
        assert g0.keys() == g1.keys()
        for k in g0:  # (printed for the record: elements that differ, of how many)
            print(f"  {name} {k}: {int((g0[k] != g1[k]).sum())} of {g0[k].numel()} differ")
        if name == "two_strip":
            assert (g0["colors"].abs().sum(-1) > 0).sum() > P  # most Gaussians of both frames get one
            for k in g0:
                assert torch.equal(g0[k], g1[k]), k


# ----------------------------------------------------------------------------- 5. capacity overflow

def test_capacity_overflow_fills_nan_as_the_full_call():
    """R_capacity below the instance count: nothing is binned, colour and inverse depth are NaN and
    the overflow flag is set, forward-only exactly as full."""
    from guava_renderer_amd._lib import CapacityError
    from guava_renderer_amd.batch import BatchRasterizer
    B, W, H = 2, 160, 128
    args = list(_cloud_args(W, H)) + [_backgrounds(B, "random")]
    r = BatchRasterizer(B, 6000, W, H, R_capacity=1000, device=DEV)

    def run(**kw):
        _poison(r)
        out = [x.clone() for x in r.forward(*args, **kw)]
        torch.cuda.synchronize()
        st, flag = r.status(), int(r.overflow_flag().item())
        with pytest.raises(CapacityError):
            r.poll(wait=True)
        return out, st, flag
    ref, st_ref, flag_ref = run()
    got, st_got, flag_got = run(forward_only=True)
    assert st_ref[1] and st_ref[0] > 1000 and flag_ref == 1
    assert st_got == st_ref and flag_got == flag_ref
    for a, b in zip(ref[:2], got[:2]):
        assert torch.isnan(a).all() and torch.isnan(b).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ref[2], got[2])


# ----------------------------------------------------------------------------- 6. the call the bench makes

def test_avatar_pipeline_render_equals_deform_plus_full_forward():
    """AvatarPipeline.render (deform, then BatchRasterizer.forward(forward_only=True)) at B = 4 on the
    small avatar of deform_cases equals deform + the full forward bit for bit."""
    from guava_renderer_amd import deform, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    from guava_renderer_amd.pipeline import AvatarPipeline
    V, F, N, B, W = 400, 600, 1500, 4, 96
    c = deform_cases.make_case(3, V, F, N, B)

    class SmallAvatar(AvatarPipeline):
        """AvatarPipeline on a posed mesh given directly (no EHM assets): render() is the class's own."""

        def __init__(self):
            self.dev = DEV
            self.gauss = deform.GaussianDeformer(
                {"rotations": _t(c["vtx_rotations"]), "scales": _t(c["vtx_scales"]),
                 "opacities": _t(c["opacities"][:V]), "colors": _t(c["colors"][:V])},
                {"rotations": _t(c["uv_rotations"]), "scales": _t(c["uv_scales"]),
                 "opacities": _t(c["opacities"][V:]), "colors": _t(c["colors"][V:]),
                 "local_pos": _t(c["local_xyz"]), "binding_face": _t(c["binding_face"]),
                 "face_bary": _t(c["face_bary"])}, _t(c["faces"]), apply_rgb_sigmoid=False)
            self.P = V + N
            self.B, self.W, self.H = B, W, W
            self.rast = BatchRasterizer(B, self.P, W, W, R_capacity=64 * self.P * B, device=DEV)
            self.bg = torch.zeros((B, C), dtype=torch.float32, device=DEV)
            self.verts, self.vt = _t(c["verts"]), _t(c["vert_transforms"])

        def deform(self, body_params, flame_params):
            return self.gauss(self.verts, self.vt)

    pipe = SmallAvatar()
    cams = _cam_args(scenes.frame_cameras(B, W, W, seed=5))
    _poison(pipe.rast)
    col, inv, radii, d = pipe.render(None, None, *cams)
    torch.cuda.synchronize()
    R_got, ovf = pipe.rast.status()
    assert not ovf and (radii > 0).sum() > pipe.P * B // 2
    d2 = pipe.gauss(pipe.verts, pipe.vt)
    for k in ("xyz", "rotation", "scaling"):
        assert torch.equal(d[k], d2[k]), k
    full = BatchRasterizer(B, pipe.P, W, W, R_capacity=64 * pipe.P * B, device=DEV)
    _poison(full)
    ref = full.forward(d2["xyz"], pipe.gauss.colors, pipe.gauss.opacity, d2["scaling"], d2["rotation"], *cams, pipe.bg)
    torch.cuda.synchronize()
    _assert_same(ref, full.status()[0], (col, inv, radii), R_got)
