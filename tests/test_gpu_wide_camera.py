"""Wide-angle and close cameras on the GPU: the EWA clamp, the near plane, unequal fields of view.

Every other GPU test sees its scene through camera.camera (tanfovx == tanfovy == 1 / 24, distance
22), where computeCov2D's clamp of t.xy / t.z never acts, no Gaussian comes nearer than z = 21 and the
perspective column of the projection's Jacobian is next to nothing.  Here:

* helpers.wide_scene: tanfov (0.8, 0.5) at distance 1.6 -- Gaussians beyond the clamp's limit on
  either axis or both (preprocess_dev.h computeCov2D; x_grad_mul / y_grad_mul and the clamped t.x, t.y
  of the tz^3 terms in preprocess_bwd.hip), footprints of a hundred pixels, means far off screen,
  non-unit quaternions;
* helpers.near_scene: tanfov 0.6 at distance 0.5 -- Gaussians on both sides of the near plane in one
  frame, rows within a few ulp of z = 0.2f, a hundred visible ones at z 0.2..0.4;
* a batch of three frames with a different tanfov row, yaw and distance each.

Forward: bit-exact with the oracle.  Backward: against the oracle by helpers.grad_check at its bars,
and directly against float64 autograd (tests/torch_ref.py) at GRAD_SCALE_TOL.  The references are
computed once per scene (_reference), with the scene's conditions (helpers.wide_conditions /
near_conditions) asserted from the oracle and float64 alone before anything of the GPU's is looked
at; tests/test_oracle.py pins the oracle on the same scenes and shows, from float64 alone, that the
clamp, the order of its two limits and the perspective column each move the gradients by more than
0.1 of their scale.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import (F64_NAMES, GRAD_SCALE_TOL, float64_reference, fov_camera, gpu_forward,
                     grad_check, near_conditions, near_scene, oracle_forward, scale_err, view_space, wide_cloud,
                     wide_conditions, wide_scene)
from test_gpu_backward import NAMES, _gpu_backward, _oracle_backward
from test_gpu_forward import _compare_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = 32

SCENES = [("wide", False), ("wide", True), ("near", False)]
IDS = ["wide", "wide-aa", "near"]


@functools.lru_cache(maxsize=None)
def _reference(name, aa):
    """The scene, its cotangents, the oracle's forward and gradients (and the gradients accumulated
    in reverse order), float64's image, n_contrib and gradients -- computed once, left unchanged."""
    d, dL, dLinv = wide_scene() if name == "wide" else near_scene()
    o_col, o_radii, o_inv, st = oracle_forward(d, antialiasing=aa)
    img, nc, f64 = float64_reference(d, st, dL, dLinv, antialiasing=aa)
    assert (nc == st["n_contrib"]).all()
    if name == "wide":
        wide_conditions(d, o_radii, f64["means3D"])
    else:
        near_conditions(d, o_radii)
    o = _oracle_backward(d, dL, dLinv, antialiasing=aa)
    o_rev = _oracle_backward(d, dL, dLinv, antialiasing=aa, reverse_order=True)
    return dict(d=d, dL=dL, dLinv=dLinv, o_col=o_col, o_radii=o_radii, st=st, img=img, f64=f64, o=o, o_rev=o_rev)


def _pick(x):
    return dict(colors=x[1], opacity=x[2].reshape(-1), means3D=x[3], scales=x[6], rotations=x[7], means2D=x[0][:, :2])


# ---------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("name,aa", SCENES, ids=IDS)
def test_forward_bit_exact(name, aa):
    """_C.rasterize_gaussians (the quad kernel): radii, tile counts, depth, means2D, conic, the sorted
    lists and ranges, n_contrib, final_T, image and inverse depth, bit for bit."""
    r = _reference(name, aa)
    gs, os_ = _compare_exact(r["d"], antialiasing=aa)
    assert gs["R"] > 0 and (os_["n_contrib"] > 0).any()


def test_forward_many_blocks_bit_exact():
    """The wide recipe at P = 4000 and 128x96: sixteen blocks of Gaussians for the scan and the
    binning, radii of two hundred pixels and means far off screen on every side (get_rect clamps
    at both ends), against the oracle alone."""
    d, _, _ = wide_scene(P=4000, W=128, H=96)
    gs, os_ = _compare_exact(d)
    t = view_space(d)
    vis = os_["radii"] > 0
    px = os_["means2D"][vis]
    assert os_["radii"].max() > 128 and vis.sum() > 2000
    assert (px[:, 0] < 0).any() and (px[:, 0] > 128).any() and (px[:, 1] < 0).any() and (px[:, 1] > 96).any()
    assert (vis & (np.abs(t[:, 0] / t[:, 2]) > 1.3 * d["tanfovx"])).sum() > 100


MIXED = [dict(tanfovx=0.8, tanfovy=0.5, yaw=0.3, pitch=-0.2, distance=1.6),
         dict(tanfovx=0.5, tanfovy=0.8, yaw=-0.25, pitch=0.15, distance=1.9),
         dict(tanfovx=0.6, tanfovy=0.6, yaw=0.1, pitch=0.0, distance=1.3)]


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


@functools.lru_cache(maxsize=None)
def _mixed_batch(P, W, H):
    """wide_cloud under three cameras with a tanfov row each: (cloud, cameras, backgrounds [3,32],
    the oracle's forward per frame).  From the oracle alone: every frame clamps at least ten visible
    Gaussians, and would clamp ten others under another frame's tanfov row."""
    import oracle
    sc = wide_cloud(P)
    cams = [fov_camera(W, H, **kw) for kw in MIXED]
    bgs = np.random.default_rng(4).uniform(-1.0, 2.0, (len(cams), C)).astype(np.float32)
    fwd = []
    for f, cam in enumerate(cams):
        o = oracle.forward(sc["means3D"], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"], None,
                           cam["viewmatrix"], cam["projmatrix"], W, H, cam["tanfovx"], cam["tanfovy"], bgs[f])
        t = view_space(dict(sc, **cam))
        ax, ay = np.abs(t[:, 0] / t[:, 2]), np.abs(t[:, 1] / t[:, 2])
        vis = o[1] > 0
        mine = (ax > 1.3 * cam["tanfovx"]) | (ay > 1.3 * cam["tanfovy"])
        assert (vis & mine).sum() >= 10, f
        for other in cams[:f] + cams[f + 1:]:
            theirs = (ax > 1.3 * other["tanfovx"]) | (ay > 1.3 * other["tanfovy"])
            assert (vis & (mine != theirs)).sum() >= 10, f
        fwd.append(o)
    return sc, cams, bgs, fwd


def _mixed_args(sc, cams, bgs):
    args = [_t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")]
    args.append(_t(np.stack([c["viewmatrix"].reshape(16) for c in cams])))
    args.append(_t(np.stack([c["projmatrix"].reshape(16) for c in cams])))
    tanf = np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32)
    assert len({tuple(r) for r in tanf}) == len(cams) and (tanf[:, 0] != tanf[:, 1]).any()
    return args + [_t(tanf), _t(bgs)]


@pytest.mark.parametrize("P,W,H", [(400, 64, 48), (4000, 128, 96)])
def test_batch_forward_tanfov_row_per_frame_bit_exact(P, W, H):
    """BatchRasterizer.forward, B = 3, in.tan_dev[2 b], [2 b + 1] different in every frame: each
    frame's image, inverse depth and radii equal its own oracle call, and the forward-only
    instantiation gives the same bits."""
    from guava_renderer_amd.batch import BatchRasterizer
    sc, cams, bgs, fwd = _mixed_batch(P, W, H)
    args = _mixed_args(sc, cams, bgs)
    r = BatchRasterizer(len(cams), P, W, H, R_capacity=48 * P * len(cams), device=DEV)
    full = [x.clone() for x in r.forward(*args)]
    torch.cuda.synchronize()
    R_full, ovf = r.status()
    assert not ovf and R_full == sum(o[3]["R"] for o in fwd)
    for x in r.out_color, r.out_invdepth:
        x.fill_(7.0)
    r.radii.fill_(-7)
    only = [x.clone() for x in r.forward(*args, forward_only=True)]
    torch.cuda.synchronize()
    assert r.status()[0] == R_full
    for got in (full, only):
        col, inv, radii = (x.cpu().numpy() for x in got)
        for f, (o_col, o_radii, o_inv, _) in enumerate(fwd):
            np.testing.assert_array_equal(radii[f], o_radii)
            np.testing.assert_array_equal(col[f], o_col)
            np.testing.assert_array_equal(inv[f], o_inv.reshape(H, W))


# --------------------------------------------------------------------------------------- backward

@pytest.mark.parametrize("name,aa", SCENES, ids=IDS)
def test_backward_matches_oracle(name, aa):
    """_C.rasterize_gaussians_backward against the oracle at grad_check's bars; the rows of every
    culled Gaussian -- in the near scene a hundred of them by the near plane, beside visible ones at
    z 0.2..0.4 -- are exactly zero."""
    r = _reference(name, aa)
    g = _gpu_backward(r["d"], r["dL"], r["dLinv"], antialiasing=aa)
    for n, a, b, bn in zip(NAMES, g, r["o"], r["o_rev"]):
        if b.size:
            grad_check(n, a, b, noise=bn)
    culled = r["o_radii"] == 0
    assert culled.sum() >= 50
    for n, a in zip(NAMES, g):
        if a.size:
            assert not a.reshape(len(culled), -1)[culled].any(), n


@pytest.mark.parametrize("name,aa", SCENES, ids=IDS)
def test_gpu_matches_float64_autograd(name, aa):
    """The GPU's image and gradients directly against float64 autograd over the same tile lists, at
    the numerics contract's bars, with the oracle's error beside them."""
    r = _reference(name, aa)
    d, st, ref = r["d"], r["st"], r["f64"]
    g_col, _, _, gs = gpu_forward(d, antialiasing=aa)
    np.testing.assert_array_equal(gs["n_contrib"], st["n_contrib"])
    err_g, err_o = np.abs(r["img"] - g_col).max(), np.abs(r["img"] - r["o_col"]).max()
    print(f"  image vs float64: GPU {err_g:.3g}, oracle {err_o:.3g}")
    assert err_g < 2e-5, err_g
    gg, oo = _pick(_gpu_backward(d, r["dL"], r["dLinv"], antialiasing=aa)), _pick(r["o"])
    errs = {n: (scale_err(gg[n], ref[n]), scale_err(oo[n], ref[n])) for n in F64_NAMES}
    for n, (eg, eo) in errs.items():
        print(f"  {n} vs float64, of scale: GPU {eg:.3g}, oracle {eo:.3g}")
    for n, (eg, _) in errs.items():
        assert np.abs(ref[n]).max() > 0, n
        assert eg <= GRAD_SCALE_TOL, f"{n}: {eg:.3g} of scale"


def test_backward_split_bf16():
    """The wide scene with the g contraction on split-bf16 MFMAs, at test_backward_bg_split_bf16's
    bars."""
    from guava_renderer_amd import _lib
    r = _reference("wide", False)
    g = _gpu_backward(r["d"], r["dL"], r["dLinv"], numerics=_lib.numerics(split_bf16=True))
    for n, a, b, bn in zip(NAMES, g, r["o"], r["o_rev"]):
        if b.size:
            grad_check(n, a, b, noise=bn, p999_tol=5e-4)


def test_batch_backward_tanfov_row_per_frame():
    """BatchRasterizer.backward on the three-frame batch: every frame against the oracle run with
    that frame's tanfov, and the frame-summed entry (shared=True) against the sum of the per-frame
    result at test_batch_backward_per_frame_backgrounds_and_shared_sum's 1e-5."""
    from guava_renderer_amd.batch import BatchRasterizer
    P, W, H = 400, 64, 48
    sc, cams, bgs, _ = _mixed_batch(P, W, H)
    B = len(cams)
    args = _mixed_args(sc, cams, bgs)
    rng = np.random.default_rng(8)
    dL = rng.normal(size=(B, C, H, W)).astype(np.float32)
    dLinv = rng.normal(size=(B, H, W)).astype(np.float32)
    r = BatchRasterizer(B, P, W, H, R_capacity=48 * P * B, device=DEV)
    r.forward(*args)
    per = r.backward(*args, _t(dL), _t(dLinv))
    sh = r.backward(*args, _t(dL), _t(dLinv), shared=True)
    torch.cuda.synchronize()
    assert not r.status()[1]
    gpu = {k: v.cpu().numpy() for k, v in per.items() if v is not None}
    for f, cam in enumerate(cams):
        print(f"frame {f}:")
        d = dict(sc, **cam, bg=bgs[f])
        o = _oracle_backward(d, dL[f], dLinv[f][None])
        o_rev = _oracle_backward(d, dL[f], dLinv[f][None], reverse_order=True)
        mine = {"means2D": gpu["mean2D"][f], "colors": gpu["colors"][f], "opacity": gpu["opacity"][f],
                "means3D": gpu["means3D"][f], "cov3D": gpu["cov3D"][f], "scales": gpu["scales"][f],
                "rotations": gpu["rotations"][f]}
        for n, b, bn in zip(NAMES, o, o_rev):
            if n in mine:
                assert np.abs(b).max() > 0, n
                grad_check(f"frame {f} {n}", mine[n], b, noise=bn)
    for k in ("means3D", "colors", "opacity", "scales", "rotations"):
        err = scale_err(sh[k].cpu().numpy(), gpu[k].sum(0))
        print(f"  shared {k}: {err:.3g} of scale")
        assert err <= 1e-5, f"{k}: {err:.3g}"
