"""The operand axes every other GPU test holds at their trivial value: a non-zero background, a
scale modifier != 1, antialiasing in the backward, and image sizes that are no multiple of the tile
in the backward.

* forward (single frame and batched, per-frame and broadcast backgrounds): bit-exact with the oracle;
* backward (single frame, batched per-frame and frame-summed, precomputed cov3D, ragged images, empty
  and one-Gaussian frames): every gradient against the oracle by helpers.grad_check at its bars;
* the six small scenes of helpers.OPERAND_SCENES, on which tests/test_oracle.py pins the oracle to
  float64 autograd (tests/torch_ref.py): the GPU directly against float64, at GRAD_SCALE_TOL.

Every reference is computed once per scene (_reference) together with a sensitivity check from the
oracle alone: the term under test moves the gradients it touches by at least 1e-2 of their scale,
100x the bar, so a kernel without that term cannot pass.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import (F64_NAMES, GRAD_SCALE_TOL, OPERAND_SCENES, float64_reference, gpu_forward, grad_check,
                     make_scene, operand_scene, oracle_forward, scale_err, torch_inputs)
from test_gpu_backward import NAMES, _gpu_backward, _oracle_backward
from test_gpu_forward import _compare_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 32
SENSITIVITY = 1e-2  # of scale: 100x GRAD_SCALE_TOL


def _bg(shape=(C,), seed=3):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, shape).astype(np.float32)


def _scene(kind, P, W, H, seed, yaw=0.0, pitch=0.0, xy=None):
    d = make_scene(kind, P, W, H, seed=seed, yaw=yaw, pitch=pitch)
    if xy is not None:
        d["means3D"][:, :2] *= np.float32(xy)
    d["bg"] = _bg()
    return d


def _cotangents(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(C, H, W)).astype(np.float32), rng.normal(size=(1, H, W)).astype(np.float32)


def _sensitivity(d, dL, dLinv, mod, aa, o):
    """From the oracle alone: what the gradients `o` would be without the operand under test."""
    kw = dict(scale_modifier=mod, antialiasing=aa)
    # (a) the background term of dL/dalpha reaches the opacity and the 2D mean
    z = _oracle_backward(dict(d, bg=np.zeros(C, np.float32)), dL, dLinv, **kw)
    for i in (0, 2):
        e = scale_err(z[i], o[i])
        print(f"  sensitivity: {NAMES[i]} with bg = 0 differs by {e:.3g} of scale")
        assert e >= SENSITIVITY, (NAMES[i], e)
    if mod != 1.0:
        # (b) the modifier changes the scales gradient by more than the factor a gradient w.r.t.
        # the unmodified scales would carry
        one = _oracle_backward(d, dL, dLinv, antialiasing=aa)
        e = scale_err(one[6] / mod, o[6])
        print(f"  sensitivity: scales at mod 1.0 / {mod} differs by {e:.3g} of scale; times mod by {abs(1 - mod):.3g}")
        assert e >= SENSITIVITY and abs(1 - mod) >= SENSITIVITY, e
    if aa:
        # (c) the antialiasing term of the covariance backward
        import oracle
        _, _, _, st = oracle_forward(d, **kw)
        off = oracle.backward(st, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], None,
                              d["viewmatrix"], d["projmatrix"], d["image_width"], d["image_height"],
                              d["tanfovx"], d["tanfovy"], d["bg"], dL, dLinv, scale_modifier=mod,
                              antialiasing=False)
        e = scale_err(off[6], o[6])
        print(f"  sensitivity: scales with the backward's antialiasing off differs by {e:.3g} of scale")
        assert e >= SENSITIVITY, e


def _with_reference(d, dL, dLinv, mod, aa):
    kw = dict(scale_modifier=mod, antialiasing=aa)
    o = _oracle_backward(d, dL, dLinv, **kw)
    _sensitivity(d, dL, dLinv, mod, aa, o)
    return d, dL, dLinv, o, _oracle_backward(d, dL, dLinv, reverse_order=True, **kw)


@functools.lru_cache(maxsize=None)
def _reference(kind, P, W, H, seed, mod=1.0, aa=False, yaw=0.0, pitch=0.0, xy=None):
    """(scene with a non-zero bg, dL, dLinv, oracle gradients, the same accumulated in reverse order),
    computed once per scene and left unchanged by the tests that share it."""
    return _with_reference(_scene(kind, P, W, H, seed, yaw, pitch, xy), *_cotangents(W, H, seed), mod, aa)


def _check_backward(ref, mod=1.0, aa=False, numerics=0, p999_tol=None):
    d, dL, dLinv, o, o_rev = ref
    g = _gpu_backward(d, dL, dLinv, antialiasing=aa, numerics=numerics, scale_modifier=mod)
    for name, a, b, bn in zip(NAMES, g, o, o_rev):
        if b.size:
            grad_check(name, a, b, noise=bn, p999_tol=p999_tol)


# ---------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("mod,aa", [(0.6, False), (1.7, False), (1.7, True)])
def test_forward_bg_and_scale_modifier_bit_exact(mod, aa):
    """C + T bg over real content, and cov3d_fwd's modifier, against the oracle."""
    d = _scene("random", 3000, 128, 96, seed=3)
    gs, os_ = _compare_exact(d, antialiasing=aa, scale_modifier=mod)
    _, _, _, one = oracle_forward(d, antialiasing=aa)
    assert not np.array_equal(one["radii"], os_["radii"])  # the modifier moved the footprints
    assert (os_["final_T"] > 0.5).any() and (os_["n_contrib"] > 0).any()


def _batch_vs_oracle(kind, P, W, H, seed, bgs, scale_modifier, antialiasing=False, yaw=(0.0, 0.25, -0.3),
                     broadcast=False):
    """test_gpu_forward._batch_vs_oracle with per-frame backgrounds [B,32] and a scale modifier;
    broadcast: the background handed over as the stride-0 row bgs[:1].expand(B, -1)."""
    from guava_renderer_amd import camera, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    import oracle
    sc = scenes.random_cloud(P, seed) if kind == "random" else scenes.avatar_cloud(P, seed)
    cams = [camera.camera(W, H, yaw=y, pitch=-0.5 * y) for y in yaw]
    B = len(cams)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    bg_t = t(bgs)
    if broadcast:
        bg_t = bg_t[:1].expand(B, -1)
        assert bg_t.stride(0) == 0
        bgs = np.broadcast_to(bgs[:1], bgs.shape)
    r = BatchRasterizer(B, P, W, H, R_capacity=40 * P * B, device=DEV)
    out = r.forward(*args, views, projs, tanf, bg_t, scale_modifier=scale_modifier, antialiasing=antialiasing)
    col, inv, radii = (x.cpu().numpy() for x in out)
    assert not r.status()[1]
    for f, c in enumerate(cams):
        o_col, o_radii, o_inv, _ = oracle.forward(sc["means3D"], sc["colors"], sc["opacities"], sc["scales"],
                                                  sc["rotations"], None, c["viewmatrix"], c["projmatrix"], W, H,
                                                  c["tanfovx"], c["tanfovy"], bgs[f], scale_modifier=scale_modifier,
                                                  antialiasing=antialiasing)
        np.testing.assert_array_equal(radii[f], o_radii)
        np.testing.assert_array_equal(col[f], o_col)
        np.testing.assert_array_equal(inv[f], o_inv.reshape(H, W))
        assert (o_radii > 0).any()


@pytest.mark.parametrize("aa,broadcast", [(False, False), (True, False), (False, True)])
def test_batch_forward_per_frame_backgrounds_bit_exact(aa, broadcast):
    """B = 3 frames, a background row per frame (or one stride-0 row), scale_modifier 1.7."""
    _batch_vs_oracle("random", 3000, 128, 96, seed=3, bgs=_bg((3, C), seed=4), scale_modifier=1.7,
                     antialiasing=aa, broadcast=broadcast)


# ------------------------------------------------------------------------- single-frame backward

SINGLE = {"random": ("random", 2000, 96, 64, 1), "avatar": ("avatar", 12000, 128, 128, 3)}


@pytest.mark.parametrize("mod,aa", [(1.0, False), (0.6, False), (1.7, False), (1.0, True)])
@pytest.mark.parametrize("scene", sorted(SINGLE))
def test_backward_bg_and_scale_modifier(scene, mod, aa):
    """_C.rasterize_gaussians_backward with a non-zero background: the render backward's
    -T_final (bg . dL) / (1 - alpha) term, and dL/dscales as the gradient w.r.t. mod * scales."""
    _check_backward(_reference(*SINGLE[scene], mod=mod, aa=aa), mod=mod, aa=aa)


@pytest.mark.parametrize("scene", sorted(SINGLE))
def test_backward_bg_split_bf16(scene):
    """The same with the g contraction on split-bf16 MFMAs; the per-element tail bar is
    test_fullsize_backward_batch6's."""
    from guava_renderer_amd import _lib
    _check_backward(_reference(*SINGLE[scene]), numerics=_lib.numerics(split_bf16=True), p999_tol=5e-4)


def test_backward_precomputed_cov3D_ignores_scale_modifier():
    """With cov3D given, the modifier has nothing to act on: image and gradients at 1.7 are those
    at 1.0, and the scales and rotations gradients are exactly zero."""
    import oracle
    d = _scene("random", 2000, 80, 80, seed=6)
    st = oracle.preprocess(d["means3D"], d["scales"], d["rotations"], d["opacities"], None,
                           d["viewmatrix"], d["projmatrix"], 80, 80, d["tanfovx"], d["tanfovy"])
    cov = st["cov3D"].copy()
    dL, dLinv = _cotangents(80, 80, 6)
    o = _oracle_backward(d, dL, dLinv, use_cov=cov)
    o_rev = _oracle_backward(d, dL, dLinv, use_cov=cov, reverse_order=True)
    g_col, g_radii, _, _ = gpu_forward(d, use_cov=cov, scale_modifier=1.7)
    o_col, o_radii, _, _ = oracle_forward(d, use_cov=True)
    np.testing.assert_array_equal(g_radii, o_radii)
    np.testing.assert_array_equal(g_col, o_col)
    g = _gpu_backward(d, dL, dLinv, use_cov=cov, scale_modifier=1.7)
    for name, a, b, bn in zip(NAMES, g, o, o_rev):
        if b.size and name not in ("scales", "rotations"):
            grad_check(name, a, b, noise=bn)
    assert g[6].shape == (2000, 3) and g[7].shape == (2000, 4)
    assert np.all(g[6] == 0) and np.all(g[7] == 0)


# -------------------------------------------------------------------------------- ragged backward

RAGGED = [("random", 3000, 100, 70, 25, 0.0, 0.0, None), ("avatar", 15000, 150, 101, 7, 0.3, -0.2, None),
          ("random", 200, 17, 33, 25, 0.0, 0.0, None), ("random", 200, 8, 8, 25, 0.0, 0.0, None),
          ("random", 30, 1, 1, 9, 0.0, 0.0, 4.0)]


@pytest.mark.parametrize("kind,P,W,H,seed,yaw,pitch,xy", RAGGED, ids=[f"{r[0]}{r[2]}x{r[3]}" for r in RAGGED])
def test_backward_ragged_image(kind, P, W, H, seed, yaw, pitch, xy):
    """W and H that are no multiple of 16 (nor of the backward's 8x8 strips), and below one tile:
    the `inside` masks of k_render_bwd.  At 1x1 the cloud is spread (xy x 4) so that the one pixel
    ends at T = 0.52 over 20 contributors: left as it is, the pixel saturates (T = 1e-4) and the
    background term is worth 3e-5 of scale, below every bar."""
    ref = _reference(kind, P, W, H, seed, yaw=yaw, pitch=pitch, xy=xy)
    assert np.abs(ref[3][1]).max() > 0  # something was rendered
    _check_backward(ref)


# ------------------------------------------------------------------------------- batched backward

def test_batch_backward_per_frame_backgrounds_and_shared_sum():
    """BatchRasterizer.backward, B = 3 cameras, a background row per frame (the kernel's
    in.s_bg * b), scale_modifier 0.6: every frame against the oracle, and the frame-summed entry
    (shared=True) against the sum of the per-frame result."""
    from guava_renderer_amd import camera, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    B, P, W, H, mod = 3, 8000, 96, 80, 0.6
    sc = scenes.avatar_cloud(P, seed=8)
    cams = [camera.camera(W, H, yaw=y, pitch=-0.5 * y) for y in (0.0, 0.25, -0.3)]
    bgs = _bg((B, C), seed=4)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), device=DEV)  # noqa: E731
    views = t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    args = [t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    rng = np.random.default_rng(8)
    dL = rng.normal(size=(B, C, H, W)).astype(np.float32)
    dLinv = rng.normal(size=(B, H, W)).astype(np.float32)
    r = BatchRasterizer(B, P, W, H, R_capacity=40 * P * B, device=DEV)
    r.forward(*args, views, projs, tanf, t(bgs), scale_modifier=mod)
    per = r.backward(*args, views, projs, tanf, t(bgs), t(dL), t(dLinv), scale_modifier=mod)
    sh = r.backward(*args, views, projs, tanf, t(bgs), t(dL), t(dLinv), scale_modifier=mod, shared=True)
    torch.cuda.synchronize()
    assert not r.status()[1]
    gpu = {k: v.cpu().numpy() for k, v in per.items() if v is not None}
    for f, cam in enumerate(cams):
        print(f"frame {f}:")
        _, _, _, o, o_rev = _with_reference(dict(sc, **cam, bg=bgs[f]), dL[f], dLinv[f][None], mod, False)
        mine = {"means2D": gpu["mean2D"][f], "colors": gpu["colors"][f], "opacity": gpu["opacity"][f],
                "means3D": gpu["means3D"][f], "cov3D": gpu["cov3D"][f], "scales": gpu["scales"][f],
                "rotations": gpu["rotations"][f]}
        for name, b, bn in zip(NAMES, o, o_rev):
            if name in mine:
                grad_check(f"frame {f} {name}", mine[name], b, noise=bn)
    for k in ("means3D", "colors", "opacity", "scales", "rotations"):
        err = scale_err(sh[k].cpu().numpy(), gpu[k].sum(0))
        print(f"  shared {k}: {err:.3g} of scale")
        assert err <= 1e-5, f"{k}: {err:.3g}"


# ------------------------------------------------------------------------------------- empty work

SHAPES = {"means2D": 3, "colors": C, "opacity": 1, "means3D": 3, "cov3D": 6, "scales": 3, "rotations": 4}


def test_backward_after_all_culled_forward_is_zero():
    """test_all_culled_frame_is_background's scene (R = 0) with a non-zero dL and background: no
    error, gradients of the right shapes, all exactly zero -- through _C and the batched entry."""
    from guava_renderer_amd.batch import BatchRasterizer
    from test_gpu_api_edges import _world_z_for_view_z
    P, W, H = 3000, 80, 48
    d = make_scene("random", P, W, H, seed=22)
    d["means3D"][:, 2] = _world_z_for_view_z(d, d["means3D"], np.full(P, -3.0))  # all behind the camera
    d["bg"] = np.linspace(-1.0, 2.0, C).astype(np.float32)
    dL, dLinv = _cotangents(W, H, 22)
    _, radii, _, st = oracle_forward(d)
    assert st["R"] == 0 and (radii == 0).all()
    g = _gpu_backward(d, dL, dLinv)
    for name, a in zip(NAMES, g):
        if name in SHAPES:
            assert a.shape == (P, SHAPES[name]), (name, a.shape)
            assert np.all(a == 0), name
    t = torch_inputs(d)
    view = t["viewmatrix"].reshape(1, 16).expand(2, 16).contiguous()
    proj = t["projmatrix"].reshape(1, 16).expand(2, 16).contiguous()
    tanf = torch.tensor([[d["tanfovx"], d["tanfovy"]]] * 2, device=DEV)
    args = (t["means3D"], t["colors"], t["opacities"], t["scales"], t["rotations"], view, proj, tanf, t["bg"])
    r = BatchRasterizer(2, P, W, H, R_capacity=1024, device=DEV)
    r.forward(*args)
    dLb = torch.tensor(np.stack([dL, dL]), device=DEV)
    dLib = torch.tensor(np.concatenate([dLinv, dLinv]), device=DEV)
    per = r.backward(*args, dLb, dLib)
    sh = r.backward(*args, dLb, dLib, shared=True)
    r.poll(wait=True)
    for name, k in SHAPES.items():
        a = per["mean2D" if name == "means2D" else name]
        assert tuple(a.shape) == (2, P, k) and not a.any(), name
    for name in ("means3D", "colors", "opacity", "scales", "rotations"):
        assert tuple(sh[name].shape) == (P, SHAPES[name]) and not sh[name].any(), name


def test_backward_one_visible_gaussian():
    """P = 1: one Gaussian at the camera's look-at point, against the oracle."""
    W, H = 40, 24
    d = make_scene("random", 1, W, H, seed=1)
    d["means3D"][:] = (0.0, -0.6, 0.0)
    d["scales"][:] = (0.05, 0.03, 0.04)
    d["opacities"][:] = 0.8
    d["bg"] = _bg()
    dL, dLinv = _cotangents(W, H, 1)
    _, radii, _, st = oracle_forward(d)
    assert radii[0] > 0 and st["n_contrib"].any()
    _check_backward(_with_reference(d, dL, dLinv, 1.0, False))


# --------------------------------------------------------------------------- GPU against float64

@pytest.mark.parametrize("row", OPERAND_SCENES, ids=[r[0] for r in OPERAND_SCENES])
def test_gpu_matches_float64_autograd(row):
    """The GPU's image and gradients against float64 autograd over the same tile lists, at the
    numerics contract's 1e-4 of each gradient's scale, with the oracle's error beside it."""
    d, dL, dLinv, mod, aa = operand_scene(row)
    W, H = d["image_width"], d["image_height"]
    kw = dict(scale_modifier=mod, antialiasing=aa)
    g_col, _, _, gs = gpu_forward(d, **kw)
    o_col, _, _, os_ = oracle_forward(d, **kw)
    T = os_["ranges"].shape[0]
    assert gs["R"] == os_["R"]
    np.testing.assert_array_equal(gs["ranges"].reshape(T, 2), os_["ranges"])
    np.testing.assert_array_equal(gs["point_list"][:gs["R"]], os_["point_list"])
    img, nc, ref = float64_reference(d, os_, dL, dLinv, **kw)
    same = nc == gs["n_contrib"]
    assert same.mean() > 0.995, same.mean()
    err_g = np.abs(img - g_col).reshape(C, -1)[:, same].max()
    err_o = np.abs(img - o_col).reshape(C, -1)[:, same].max()
    print(f"  image vs float64: GPU {err_g:.3g}, oracle {err_o:.3g} (n_contrib agreement {same.mean():.4f})")
    assert err_g < 2e-5, err_g
    o = _oracle_backward(d, dL, dLinv, **kw)
    if (W, H) != (1, 1):  # that row's one pixel saturates (T = 1e-4): it stands for the image size,
        _sensitivity(d, dL, dLinv, mod, aa, o)  # test_backward_ragged_image has a 1x1 the bg reaches
    g = _gpu_backward(d, dL, dLinv, **kw)
    pick = lambda x: dict(colors=x[1], opacity=x[2].reshape(-1), means3D=x[3], scales=x[6], rotations=x[7],  # noqa: E731
                          means2D=x[0][:, :2])
    gg, oo = pick(g), pick(o)
    errs = {n: (scale_err(gg[n], ref[n]), scale_err(oo[n], ref[n])) for n in F64_NAMES}
    for n, (eg, eo) in errs.items():
        print(f"  {n} vs float64, of scale: GPU {eg:.3g}, oracle {eo:.3g}")
    for n, (eg, _) in errs.items():
        assert np.abs(ref[n]).max() > 0, n
        assert eg <= GRAD_SCALE_TOL, f"{n}: {eg:.3g} of scale"
