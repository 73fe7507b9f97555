"""CPU tests that pin the oracle (oracle/gsr_oracle.c).

The reference ships no tests or golden vectors for the rasterizer, and its CUDA
build cannot run here, so the oracle is pinned by: analytic known-answer cases, an independent
numpy restatement of the binning/sort contract, and an independent float64 torch restatement with
autograd (tests/torch_ref.py) for the forward image and every gradient.
"""
import numpy as np
import pytest

import oracle
from helpers import F64_NAMES, OPERAND_SCENES, float64_reference, make_scene, operand_scene, scale_err

C = 32


def _fwd(d, **kw):
    return oracle.forward(d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], None,
                          d["viewmatrix"], d["projmatrix"], d["image_width"], d["image_height"],
                          d["tanfovx"], d["tanfovy"], d["bg"], **kw)


def test_expf_accuracy():
    x = np.linspace(-87.0, 0.0, 20001).astype(np.float32)
    got = oracle.expf(x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    rel = np.abs(got - ref) / ref
    assert rel.max() < 3e-7, rel.max()
    assert oracle.expf([0.0])[0] == 1.0
    assert np.isnan(oracle.expf([np.nan])[0])


def test_blend_exp_accuracy():
    """The blend's exp (2^k (1 + q), gsr_oracle.c blend_parts) and alpha = fma(o 2^k, q, o 2^k):
    within 1 ulp / 1.3 ulp of float64 o exp(x) wherever alpha can reach 1/255 (x > -5.54)."""
    x = np.linspace(-5.6, 0.0, 40001).astype(np.float32)
    ref = np.exp(x.astype(np.float64))
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert (np.abs(oracle.blend_G(x) - ref) / ulp).max() <= 1.0
    for o in (1.0, 0.37, 0.99, 0.013):
        o32 = float(np.float32(o))
        ref_a = np.minimum(0.99, o32 * ref)
        ulp_a = np.spacing(ref_a.astype(np.float32)).astype(np.float64)
        assert (np.abs(oracle.blend_alpha(o32, x) - ref_a) / ulp_a).max() <= 1.3
    assert oracle.blend_alpha(0.5, [-90.0])[0] == 0.0           # never blends
    assert oracle.blend_alpha(0.5, [np.nan])[0] == np.float32(0.99)  # as min(0.99, NaN) in the reference
    assert oracle.blend_alpha(0.5, [0.0])[0] == 0.5


def _single(o=0.5, W=64, H=64, scale=0.02, off=(0.0, 0.0, 0.0), feat=None):
    from guava_renderer_amd import camera
    cam = camera.camera(W, H)
    d = dict(cam)
    d["means3D"] = np.array([[off[0], off[1] - 0.6, off[2]]], np.float32)
    d["scales"] = np.full((1, 3), scale, np.float32)
    d["rotations"] = np.array([[1, 0, 0, 0]], np.float32)
    d["opacities"] = np.array([[o]], np.float32)
    d["colors"] = (np.arange(C, dtype=np.float32)[None] / 7.0 - 1.0) if feat is None else feat
    d["bg"] = np.zeros(C, np.float32)
    return d


def test_known_answer_single_gaussian():
    d = _single(o=0.5)
    col, radii, invd, st = _fwd(d)
    assert radii[0] > 0
    mx, my = st["means2D"][0]
    co = st["conic_opacity"][0].astype(np.float64)
    H, W = col.shape[1:]
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = mx - xs, my - ys
    power = -0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
    alpha = np.minimum(0.99, co[3] * np.exp(power))
    # only pixels of tiles inside the Gaussian's rect see it
    rect_mask = np.zeros((H, W), bool)
    gx = (W + 15) // 16
    for t in range(st["ranges"].shape[0]):
        if st["ranges"][t, 1] > st["ranges"][t, 0]:
            tx, ty = t % gx, t // gx
            rect_mask[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    a = np.where(rect_mask & (alpha >= 1 / 255), alpha, 0.0)
    expect = a[None] * d["colors"][0][:, None, None]
    np.testing.assert_allclose(col, expect, atol=2e-6)
    np.testing.assert_allclose(st["final_T"].reshape(H, W), 1 - a, atol=1e-6)
    np.testing.assert_array_equal(st["n_contrib"].reshape(H, W), (a > 0).astype(np.uint32))
    # inverse depth image: alpha / z
    np.testing.assert_allclose(invd[0], a / st["depths"][0], rtol=1e-5, atol=1e-9)


def test_known_answer_two_gaussians_depth_order():
    d = _single(o=0.6, scale=0.05)
    d2 = _single(o=0.7, scale=0.05, off=(0.0, 0.0, 0.1))  # farther from the camera (+z)
    for k in ("means3D", "scales", "rotations", "opacities"):
        d[k] = np.concatenate([d2[k], d[k]], 0)  # back one first in index order
    d["colors"] = np.stack([np.full(C, 2.0, np.float32), np.full(C, 1.0, np.float32)])
    col, radii, invd, st = _fwd(d)
    H, W = col.shape[1:]
    # per tile lists are depth-sorted: the near Gaussian (index 1) comes first
    for t in range(st["ranges"].shape[0]):
        s, e = st["ranges"][t]
        if e - s == 2:
            assert list(st["point_list"][s:e]) == [1, 0]
    c = H // 2 * W + W // 2
    co = st["conic_opacity"].astype(np.float64)
    m = st["means2D"].astype(np.float64)
    a = []
    for g in (1, 0):
        dx, dy = m[g, 0] - W // 2, m[g, 1] - H // 2
        p = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
        a.append(min(0.99, co[g, 3] * np.exp(p)))
    expect = 1.0 * a[0] + 2.0 * a[1] * (1 - a[0])
    assert abs(col[0].reshape(-1)[c] - expect) < 1e-5
    assert abs(st["final_T"][c] - (1 - a[0]) * (1 - a[1])) < 1e-6


def test_saturation_stops_before_terminating_gaussian():
    # 30 opaque Gaussians stacked on the same pixel: T stops above 1e-4 and the Gaussian that would
    # push T below it is excluded (forward.cu:363-368)
    n = 30
    d = _single(o=0.99, scale=0.05)
    for k in ("means3D", "scales", "rotations", "opacities"):
        d[k] = np.repeat(d[k], n, 0)
    d["means3D"][:, 2] = np.linspace(0, 0.2, n).astype(np.float32)
    d["colors"] = np.ones((n, C), np.float32)
    col, radii, invd, st = _fwd(d)
    H, W = col.shape[1:]
    c = H // 2 * W + W // 2
    T = st["final_T"][c]
    k = int(st["n_contrib"][c])
    assert T >= 1e-4 and 0 < k < n
    # the next Gaussian in the pixel's list is the one that would push T below 1e-4: excluded
    t = (H // 2 // 16) * ((W + 15) // 16) + (W // 2 // 16)
    s, e = st["ranges"][t]
    g = int(st["point_list"][s + k])
    co = st["conic_opacity"][g].astype(np.float64)
    dx, dy = st["means2D"][g, 0] - W // 2, st["means2D"][g, 1] - H // 2
    a = min(0.99, co[3] * np.exp(-0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy))
    assert a >= 1 / 255 and T * (1 - a) < 1e-4


def test_binning_contract_independent_restatement():
    d = make_scene("random", 3000, 160, 96, seed=21)
    _, radii, _, st = _fwd(d)
    W, H = 160, 96
    gx, gy = (W + 15) // 16, (H + 15) // 16
    # independent restatement: instances from rects, ordered by (tile, depth bits, index)
    inst = []
    for g in np.nonzero(radii > 0)[0]:
        mx, my = st["means2D"][g]
        r = np.float32(radii[g])
        def cl(v, hi):
            v = int(np.trunc(v)) if np.isfinite(v) else 0
            return min(max(v, 0), hi)
        x0 = cl((mx - r) / np.float32(16), gx); x1 = cl((((mx + r) + np.float32(16)) - np.float32(1)) / np.float32(16), gx)
        y0 = cl((my - r) / np.float32(16), gy); y1 = cl((((my + r) + np.float32(16)) - np.float32(1)) / np.float32(16), gy)
        db = np.float32(st["depths"][g]).view(np.uint32)
        for y in range(y0, y1):
            for x in range(x0, x1):
                inst.append((y * gx + x, int(db), int(g)))
    inst.sort()
    assert len(inst) == st["R"]
    np.testing.assert_array_equal(np.array([i[2] for i in inst], np.uint32), st["point_list"])
    tiles = np.array([i[0] for i in inst])
    for t in range(gx * gy):
        idx = np.nonzero(tiles == t)[0]
        exp = (idx[0], idx[-1] + 1) if len(idx) else (0, 0)
        assert tuple(st["ranges"][t]) == exp


def test_equal_depth_ties_keep_index_order():
    d = make_scene("random", 500, 64, 64, seed=22)
    d["means3D"][:, 2] = 0.0  # identical depth for everyone
    _, radii, _, st = _fwd(d)
    for t in range(st["ranges"].shape[0]):
        s, e = st["ranges"][t]
        lst = st["point_list"][s:e]
        assert np.all(np.diff(lst.astype(np.int64)) > 0)


def _torch_check(d, W, H, dL=None, dLinv=None, tol_img=2e-5, tol_grad=2e-5, scale_modifier=1.0,
                 antialiasing=False):
    """The oracle against tests/torch_ref.py (float64, autograd) with the scene's own d["bg"]."""
    col, radii, invd, st = _fwd(d, scale_modifier=scale_modifier, antialiasing=antialiasing)
    out, nc, ref = float64_reference(d, st, dL, dLinv, scale_modifier=scale_modifier, antialiasing=antialiasing)
    same = (nc == st["n_contrib"])
    print(f"  n_contrib agreement {same.mean():.4f}")
    assert same.mean() > 0.995, same.mean()
    err = np.abs(out - col).reshape(C, -1)[:, same].max()
    print(f"  image: {err:.3g}")
    assert err < tol_img, err
    if dL is None:
        return
    g = oracle.backward(st, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], None,
                        d["viewmatrix"], d["projmatrix"], W, H, d["tanfovx"], d["tanfovy"], d["bg"], dL, dLinv,
                        scale_modifier=scale_modifier, antialiasing=antialiasing)
    g_m2, g_col, g_op, g_m3, g_cov, g_sh, g_sc, g_rot = g
    ours = dict(colors=g_col, opacity=g_op.reshape(-1), means3D=g_m3, scales=g_sc, rotations=g_rot,
                means2D=g_m2[:, :2])
    errs = {name: scale_err(ours[name], ref[name]) for name in F64_NAMES}
    print("  oracle vs float64, of scale: " + ", ".join(f"{k} {v:.3g}" for k, v in errs.items()))
    for name, e in errs.items():
        assert np.abs(ref[name]).max() > 0, name
        assert e < tol_grad, (name, e)


def test_forward_and_gradients_match_float64_autograd():
    W, H = 48, 32
    d = make_scene("random", 40, W, H, seed=23)
    d["means3D"][:, :2] *= 0.25
    rng = np.random.default_rng(3)
    dL = rng.normal(size=(C, H, W)).astype(np.float32)
    dLinv = rng.normal(size=(1, H, W)).astype(np.float32)
    _torch_check(d, W, H, dL, dLinv)


@pytest.mark.parametrize("row", OPERAND_SCENES, ids=[r[0] for r in OPERAND_SCENES])
def test_operand_axes_match_float64_autograd(row):
    """A non-zero background (the backward's -T_final (bg . dL) / (1 - alpha) term), scale_modifier
    != 1 (dL/dscales is the gradient w.r.t. scale_modifier * scales), antialiasing (the backward
    evaluates its closed form at the dilated covariance) and ragged / saturated / 1x1 images: the
    oracle's image and every gradient against float64 autograd, at _torch_check's bars."""
    d, dL, dLinv, mod, aa = operand_scene(row)
    assert np.abs(d["bg"]).min() > 0
    _torch_check(d, d["image_width"], d["image_height"], dL, dLinv, scale_modifier=mod, antialiasing=aa)


SENSITIVITY = 1e-2  # of scale, as tests/test_gpu_operands.py: 100x the GPU's gradient bar


def _switch_effect(d, dL, dLinv, aa, ref, **switch):
    """float64 alone: how far the means3D / scales / rotations gradients move under torch_ref.project's
    switch, of the unswitched gradients' scale."""
    _, _, _, st = _fwd(d, antialiasing=aa)
    _, _, other = float64_reference(d, st, dL, dLinv, antialiasing=aa, **switch)
    e = {k: scale_err(other[k], ref[k]) for k in ("means3D", "scales", "rotations")}
    print(f"  sensitivity: {switch} moves " + ", ".join(f"{k} by {v:.3g}" for k, v in e.items()) + " of scale")
    return e, other


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
def test_wide_camera_matches_float64_autograd(aa):
    """helpers.wide_scene: tanfovx != tanfovy, Gaussians beyond the EWA limit of either axis or both
    (computeCov2D's clamp and x_grad_mul / y_grad_mul of its backward), a perspective column of J that
    carries a third of the gradient, non-unit quaternions.  The scene's conditions, then the oracle's
    image and every gradient against float64 autograd at _torch_check's bars, then from float64
    alone: without the clamp, with the two limits swapped, or without J's perspective column the
    gradients move by >= SENSITIVITY; and autograd through clamp(t.x / t.z) * t.z (which
    differentiates the clamped value, as this file's reference did before it was corrected) is not
    what the oracle computes."""
    from helpers import wide_conditions, wide_scene
    d, dL, dLinv = wide_scene()
    W, H = d["image_width"], d["image_height"]
    assert np.abs(d["bg"]).min() > 0 and d["tanfovx"] != d["tanfovy"]
    _, radii, _, st = _fwd(d, antialiasing=aa)
    _, nc, ref = float64_reference(d, st, dL, dLinv, antialiasing=aa)
    assert (nc == st["n_contrib"]).all()
    wide_conditions(d, radii, ref["means3D"])
    _torch_check(d, W, H, dL, dLinv, antialiasing=aa)
    for switch in (dict(clamp="none"), dict(clamp="swapped"), dict(diagonal_J=True)):
        e, _ = _switch_effect(d, dL, dLinv, aa, ref, **switch)
        assert min(e.values()) >= SENSITIVITY, (switch, e)
    e, old = _switch_effect(d, dL, dLinv, aa, ref, clamp="differentiated")
    g = oracle.backward(st, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], None,
                        d["viewmatrix"], d["projmatrix"], W, H, d["tanfovx"], d["tanfovy"], d["bg"], dL, dLinv,
                        antialiasing=aa)
    err = scale_err(g[3], old["means3D"])
    print(f"  oracle means3D vs autograd through the clamped value: {err:.3g} of scale")
    assert err >= SENSITIVITY and e["means3D"] >= SENSITIVITY, (err, e)


def test_near_camera_matches_float64_autograd():
    """helpers.near_scene: Gaussians on both sides of the near plane in one frame, a hundred visible
    ones at z 0.2..0.4 (1 / t.z^2, 1 / t.z^3 of the backward 10^4 times the canonical camera's), rows
    within a few ulp of z = 0.2f.  Conditions, the oracle against float64 autograd, zero gradient rows
    for every culled Gaussian, and the perspective column's share of the gradient."""
    from helpers import near_conditions, near_scene
    d, dL, dLinv = near_scene()
    W, H = d["image_width"], d["image_height"]
    _, radii, _, st = _fwd(d)
    _, nc, ref = float64_reference(d, st, dL, dLinv)
    assert (nc == st["n_contrib"]).all()
    near_conditions(d, radii)
    _torch_check(d, W, H, dL, dLinv)
    g = oracle.backward(st, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], None,
                        d["viewmatrix"], d["projmatrix"], W, H, d["tanfovx"], d["tanfovy"], d["bg"], dL, dLinv)
    for a in g:
        if a.size:
            assert not a.reshape(len(radii), -1)[radii == 0].any()
    e, _ = _switch_effect(d, dL, dLinv, False, ref, diagonal_J=True)
    assert min(e.values()) >= SENSITIVITY, e


def test_avatar_forward_matches_float64_restatement():
    W, H = 64, 48
    d = make_scene("avatar", 400, W, H, seed=24)
    _torch_check(d, W, H)


@pytest.mark.parametrize("W,H", [(1, 1), (17, 33), (100, 70)])
def test_odd_image_sizes(W, H):
    d = make_scene("random", 200, W, H, seed=25)
    col, radii, invd, st = _fwd(d)
    assert col.shape == (C, H, W)
    assert st["final_T"].shape == (H * W,)
    assert np.isfinite(col).all()


def test_all_behind_camera_and_transparent():
    d = make_scene("random", 50, 32, 32, seed=26)
    d["means3D"][:, 2] = -30.0  # behind the camera (view z <= 0.2)
    col, radii, _, st = _fwd(d)
    assert (radii == 0).all() and st["R"] == 0
    np.testing.assert_array_equal(col, 0.0)
    d = make_scene("random", 50, 32, 32, seed=27)
    d["opacities"][:] = 1e-3  # below 1/255: never blended
    col, radii, _, st = _fwd(d)
    assert (radii > 0).any()
    np.testing.assert_array_equal(col, 0.0)
    np.testing.assert_array_equal(st["n_contrib"], 0)


def test_prefiltered_raises():
    d = make_scene("random", 20, 32, 32, seed=28)
    d["means3D"][0, 2] = -30.0
    with pytest.raises(RuntimeError):
        _fwd(d, prefiltered=True)


def test_huge_gaussian_covers_every_tile():
    d = make_scene("random", 3, 96, 64, seed=29)
    d["scales"][0] = 5.0
    _, radii, _, st = _fwd(d)
    assert st["tiles_touched"][0] == st["ranges"].shape[0]


def test_mark_visible():
    d = make_scene("random", 100, 32, 32, seed=30)
    d["means3D"][:10, 2] = -30.0
    vis = oracle.mark_visible(d["means3D"], d["viewmatrix"], d["projmatrix"])
    assert not vis[:10].any() and vis[10:].all()


def test_antialiasing_scales_opacity():
    d = make_scene("random", 300, 64, 64, seed=31)
    _, _, _, st0 = _fwd(d)
    _, _, _, st1 = _fwd(d, antialiasing=True)
    vis = st0["radii"] > 0
    assert np.all(st1["conic_opacity"][vis, 3] <= st0["conic_opacity"][vis, 3])


def test_exact_exp_vs_libm_expf_decisions():
    """The restatement's blend exp against libm expf (the reference's CUDA expf stand-in) at config
    1: the pixels whose take/stop decisions differ (oracle.decision_flips) are <= 0.1%, and every
    other pixel agrees to 1e-4 L_inf on all 32 channels (SURVEY.md §7's bar; the GPU is bit-exact
    with the exact mode, test_gpu_ref_exp.py repeats this at configs 2 and 5)."""
    from helpers import make_scene, oracle_forward
    d = make_scene("random", 10000, 256, 256, seed=1)
    c1, _, _, s1 = oracle_forward(d, exact=True)
    c2, _, _, s2 = oracle_forward(d, exact=False)
    flips = oracle.decision_flips(s1, 256, 256)
    assert flips.mean() <= 1e-3
    assert (s1["n_contrib"] != s2["n_contrib"]).mean() <= 1e-3
    err = np.abs(c1 - c2)[:, ~flips]
    assert err.max() <= 1e-4, err.max()
    # a pixel where the exps agree on every decision differs only by the alphas' rounding
    assert err.max() <= 1e-5, err.max()


@pytest.mark.parametrize("kind,P,W", [("random", 10000, 256), ("avatar", 20000, 256)])
def test_restated_vs_literal_reference_arithmetic(kind, P, W):
    """The restatement's arithmetic (fused power, polynomial exp, fmaf colour update -- bit-exact with
    the GPU) against the reference's expressions as written (oracle mode "literal": forward.cu:352
    power, libm expf for CUDA's expf, C += f alpha T, invdepth += (1/depth) alpha T, C + T bg) at
    config-1 size: decision flips <= 0.1% of the pixels, every other pixel within 1e-5 on all 32
    channels (north_star: 1e-4), final_T within 1e-6; radii and lists do not involve the blend."""
    from helpers import make_scene, oracle_forward
    d = make_scene(kind, P, W, W, seed=2)
    c1, r1, i1, s1 = oracle_forward(d, exact=True)
    c2, r2, i2, s2 = oracle_forward(d, exact=oracle.LITERAL)
    np.testing.assert_array_equal(r1, r2)
    np.testing.assert_array_equal(s1["point_list"], s2["point_list"])
    flips = oracle.decision_flips(s1, W, W, against=oracle.LITERAL)
    assert flips.mean() <= 1e-3, flips.mean()
    assert (s1["n_contrib"] != s2["n_contrib"]).mean() <= 1e-3
    keep = ~flips.reshape(-1)
    err = np.abs(c1 - c2).reshape(32, -1)[:, keep]
    assert err.max() <= 1e-5, err.max()
    assert np.abs(s1["final_T"] - s2["final_T"])[keep].max() <= 1e-6
    assert np.abs(i1 - i2).reshape(-1)[keep].max() <= 1e-5 * max(1.0, float(np.abs(i2).max()))


def test_literal_mode_is_the_reference_expression():
    """Mode "literal" evaluates forward.cu:352-391 as written: one Gaussian, one pixel, checked
    against the same expressions evaluated step by step in numpy float32 (every op rounded)."""
    from helpers import make_scene, oracle_forward
    d = make_scene("random", 1, 16, 16, seed=3)
    col, radii, invd, st = oracle_forward(d, exact=oracle.LITERAL)
    if radii[0] == 0:
        pytest.skip("the random Gaussian was culled")
    f32 = np.float32
    xy = st["means2D"].reshape(-1, 2)[0].astype(f32)
    co = st["conic_opacity"].reshape(-1, 4)[0].astype(f32)
    depth = f32(st["depths"][0])
    checked = 0
    for y in range(16):
        for x in range(16):
            dx, dy = f32(xy[0] - f32(x)), f32(xy[1] - f32(y))
            s = f32(f32(f32(co[0] * dx) * dx) + f32(f32(co[2] * dy) * dy))
            power = f32(f32(f32(-0.5) * s) - f32(f32(co[1] * dx) * dy))
            if power > 0:
                continue
            alpha = min(f32(0.99), f32(co[3] * f32(np.exp(np.float64(power)))))  # (libm-rounded expf stand-in)
            if alpha < f32(1.0) / f32(255.0):
                continue
            c0 = f32(f32(d["colors"][0, 0] * alpha) * f32(1.0))
            want = f32(c0 + f32(f32(1.0 - alpha) * f32(d["bg"][0])))
            got = col[0, y, x]
            assert abs(float(got) - float(want)) <= 2e-7 * max(1.0, abs(float(want))), (x, y, got, want)
            wi = f32(f32(f32(f32(1.0) / depth) * alpha) * f32(1.0))
            assert abs(float(invd[0, y, x]) - float(wi)) <= 2e-7 * max(1.0, abs(float(wi)))
            checked += 1
    assert checked > 0
