"""GPU tests of the differentiable Gaussian assembly (gsr_deform_gaussians_backward), the fused
rasterizer backward of a posed avatar (gsr_backward_batch_deformed) and their Python surface
(deform.deform_gaussians, BatchRasterizer.backward_deformed, train.AvatarTrainer).

Reference of every gradient: tests/deform_ref.py, float64 autograd with the mesh-derived constants
of oracle/lbs_oracle.py.  Bar: helpers.scale_err <= helpers.GRAD_SCALE_TOL (1e-4 of the tensor's max
magnitude).  Rotation gradients are compared on the Gaussians whose rotmat_to_unitquat decision
margin is >= 1e-4 in every frame (float32 may take the other branch near a tie, which flips the
sign of q and of that frame's contribution); these must be more than 99% of the Gaussians.  Every
other gradient is compared on every Gaussian."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import deform_cases
import deform_ref
from deform_cases import ATTRS, ROT_ATTRS
from helpers import GRAD_SCALE_TOL, scale_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(seed, V, F, N, B, sort=False, per_frame=()):
    """(inputs, float64 constants, float64 reference gradients by attribute name, firm-row masks):
    computed once per case and shared, never modified."""
    c = deform_cases.make_case(seed, V, F, N, B, sort_bindings=sort, per_frame=per_frame)
    k = deform_ref.Constants(c["verts"], c["vert_transforms"], c["faces"], c["binding_face"], c["face_bary"])
    ref = dict(zip(ATTRS, deform_ref.gradients(k, [c[a] for a in ATTRS], c["g_xyz"], c["g_rot"], c["g_scl"])))
    firm = (k.margin >= 1e-4).all(0)
    assert firm.mean() > 0.99, firm.mean()  # (a condition on the inputs, not a measurement)
    return c, k, ref, {"vtx_rotations": firm[:V], "uv_rotations": firm[V:]}


def _gpu_backward(c, g_xyz=None, g_rot=None, g_scl=None, wanted=ATTRS):
    """gsr_deform_gaussians_backward on the case -> ({attr: numpy gradient}, bad flag)."""
    from guava_renderer_amd import _lib, deform
    B = c["B"]
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    attrs = [_t(c[a]) for a in ATTRS]
    di, keep = deform.deform_inputs(B, _t(c["verts"]), _t(c["vert_transforms"]), _t(c["faces"]),
                                    _t(c["binding_face"]), _t(c["face_bary"]), attrs, bad)
    outs = {a: torch.full(c[a].shape, float("nan"), dtype=torch.float32, device=DEV) for a in wanted}
    dgr = _lib.DeformGrads(*[outs[a].data_ptr() if a in outs else None for a in ATTRS])
    ups = [_t(c[n] if g is None else g) for n, g in (("g_xyz", g_xyz), ("g_rot", g_rot), ("g_scl", g_scl))]
    rc = _lib.load().gsr_deform_gaussians_backward(B, ctypes.byref(di), ups[0].data_ptr(), ups[1].data_ptr(),
                                                   ups[2].data_ptr(), ctypes.byref(dgr),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "gsr_deform_gaussians_backward")
    torch.cuda.synchronize()
    return {a: o.cpu().numpy() for a, o in outs.items()}, int(bad.item())


def _compare(what, got, ref, masks, rows=None, tol=GRAD_SCALE_TOL):
    """Scale bar on every attribute in `got`; per-frame gradients ([B,n,k]) frame by frame; rotations on
    the firm rows only.  rows: optional {attr: bool row mask} of further rows to leave out (both
    sides).  Returns the worst scale_err."""
    worst = 0.0
    for a, g in got.items():
        r = np.asarray(ref[a])
        assert g.shape == r.shape, (a, g.shape, r.shape)
        keep = np.ones(r.shape[-2], bool)
        if a in ROT_ATTRS:
            keep &= masks[a]
        if rows is not None and a in rows:
            keep &= rows[a]
        frames = [(g, r)] if r.ndim == 2 else [(g[b], r[b]) for b in range(r.shape[0])]
        for b, (gb, rb) in enumerate(frames):
            assert np.isfinite(gb).all(), (what, a, b)
            e = scale_err(gb[keep], rb[keep])
            worst = max(worst, e)
            print(f"  {what} {a}{'' if r.ndim == 2 else f' frame {b}'}: {e:.3g} of scale ({int(keep.sum())} rows)")
            assert e <= tol, f"{what} {a} frame {b}: {e:.3g} of scale"
    return worst


@pytest.mark.parametrize("seed,V,F,N,B,sort", [(3, 400, 600, 1500, 3, False), (4, 400, 600, 1500, 9, False),
                                               (5, 300, 500, 1100, 9, True), (6, 70, 40, 300, 1, False)])
def test_standalone_shared_attributes(seed, V, F, N, B, sort):
    """Shared attributes: [n,k] frame sums.  Unsorted bindings (face runs > 256 per block: per-Gaussian
    face frames), V no multiple of 256 (both kinds in one workgroup), B = 9 past the forward's 8-frame
    group; texel order (runs 54-120) and a single small frame."""
    c, k, ref, masks = _case(seed, V, F, N, B, sort)
    got, bad = _gpu_backward(c)
    assert bad == 0
    worst = _compare(f"seed {seed}", got, ref, masks)
    print(f"  seed {seed}: worst {worst:.3g}")
    # with a subset wanted, the others stay untouched and the wanted ones are the same bits
    some, _ = _gpu_backward(c, wanted=("vtx_scales", "uv_rotations"))
    assert set(some) == {"vtx_scales", "uv_rotations"}
    for a in some:
        assert np.array_equal(some[a], got[a]), a


@pytest.mark.parametrize("per_frame", [ATTRS, ("local_xyz",)])
def test_standalone_per_frame_attributes(per_frame):
    """[B,n,k] attributes at B = 9: one gradient row per frame, each frame compared separately; and
    the mixed case (local offsets per frame, the other attributes shared)."""
    c, k, ref, masks = _case(4, 400, 600, 1500, 9, False, per_frame)
    for a in ATTRS:
        assert c[a].ndim == (3 if a in per_frame else 2)
    got, bad = _gpu_backward(c)
    assert bad == 0
    _compare("per-frame" if len(per_frame) > 1 else "mixed", got, ref, masks)


def test_bad_binding_gets_zero_rows_and_the_flag():
    c0, k, ref, masks = _case(3, 400, 600, 1500, 3)
    c = dict(c0)
    c["binding_face"] = c0["binding_face"].copy()
    c["binding_face"][17] = c0["F"] + 3  # out of range
    got, bad = _gpu_backward(c)
    assert bad == 1
    ok = np.ones(c["N"], bool)
    ok[17] = False
    for a in ("local_xyz", "uv_rotations", "uv_scales"):
        assert np.all(got[a][17] == 0.0), a
    _compare("bad binding", got, ref, masks, rows={a: ok for a in ("local_xyz", "uv_rotations", "uv_scales")})


def _deformer(c):
    from guava_renderer_amd import deform
    V = c["V"]
    return deform.GaussianDeformer(
        {"rotations": _t(c["vtx_rotations"]), "scales": _t(c["vtx_scales"]), "opacities": _t(c["opacities"][:V]),
         "colors": _t(c["colors"][:V])},
        {"rotations": _t(c["uv_rotations"]), "scales": _t(c["uv_scales"]), "opacities": _t(c["opacities"][V:]),
         "colors": _t(c["colors"][V:]), "local_pos": _t(c["local_xyz"]), "binding_face": _t(c["binding_face"]),
         "face_bary": _t(c["face_bary"])}, _t(c["faces"]), apply_rgb_sigmoid=False)


def test_autograd_function_matches_deformer_and_reference():
    from guava_renderer_amd import deform
    c, k, ref, masks = _case(3, 400, 600, 1500, 3)
    verts, T = _t(c["verts"]), _t(c["vert_transforms"])
    d = _deformer(c)(verts, T)
    leaves = [_t(c[a]).requires_grad_(True) for a in ATTRS]
    xyz, rot, scl = deform.deform_gaussians(verts, T, _t(c["faces"]), _t(c["binding_face"]), _t(c["face_bary"]),
                                            *leaves)
    assert torch.equal(xyz, d["xyz"]) and torch.equal(rot, d["rotation"]) and torch.equal(scl, d["scaling"])
    ((xyz * _t(c["g_xyz"])).sum() + (rot * _t(c["g_rot"])).sum() + (scl * _t(c["g_scl"])).sum()).backward()
    torch.cuda.synchronize()
    _compare("autograd", {a: l.grad.cpu().numpy() for a, l in zip(ATTRS, leaves)}, ref, masks)
    # only some leaves: the others get no gradient
    lv = [_t(c[a]) for a in ATTRS]
    lv[2].requires_grad_(True)
    out = deform.deform_gaussians(verts, T, _t(c["faces"]), _t(c["binding_face"]), _t(c["face_bary"]), *lv)
    (out[0] * _t(c["g_xyz"])).sum().backward()
    assert scale_err(lv[2].grad.cpu().numpy(), ref["local_xyz"]) <= GRAD_SCALE_TOL and lv[0].grad is None
    with pytest.raises(NotImplementedError):
        deform.deform_gaussians(verts.clone().requires_grad_(True), T, _t(c["faces"]), _t(c["binding_face"]),
                                _t(c["face_bary"]), *leaves)


# ---- the rendered avatar of the fused tests: case 1's avatar (seed 3, B = 3) at 96 x 96 with one
# vertex Gaussian placed so that it is culled in frame 1 only
W = 96
CULL_V = 7


@functools.lru_cache(maxsize=None)
def _scene():
    from guava_renderer_amd import scenes
    c0, _, _, _ = _case(3, 400, 600, 1500, 3)
    c = dict(c0)
    V, B = c["V"], c["B"]
    # vertex CULL_V leaves every face (its move must not stretch a face frame), then sits near the
    # origin in frames 0 and 2 and far off screen in frame 1
    faces = c0["faces"].copy()
    for f in np.nonzero((faces == CULL_V).any(1))[0]:
        j = int(np.nonzero(faces[f] == CULL_V)[0][0])
        faces[f, j] = next(v for v in range(CULL_V + 1, V) if v not in faces[f])
    verts = c0["verts"].copy()
    verts[:, CULL_V] = (0.01, 0.02, 0.0)
    verts[1, CULL_V] = (60.0, 0.02, 0.0)
    c["faces"], c["verts"] = faces, verts
    rng = np.random.default_rng(17)
    cams = scenes.frame_cameras(B, W, W, seed=5)
    c["cams"] = cams
    c["views"] = np.stack([cm["viewmatrix"].reshape(16) for cm in cams])
    c["projs"] = np.stack([cm["projmatrix"].reshape(16) for cm in cams])
    c["tanf"] = np.array([[cm["tanfovx"], cm["tanfovy"]] for cm in cams], np.float32)
    c["bg"] = rng.uniform(0, 1, (B, 32)).astype(np.float32)
    c["dL"] = rng.normal(size=(B, 32, W, W)).astype(np.float32)
    c["dLinv"] = rng.normal(size=(B, W, W)).astype(np.float32)
    k = deform_ref.Constants(c["verts"], c["vert_transforms"], c["faces"], c["binding_face"], c["face_bary"])
    firm = (k.margin >= 1e-4).all(0)
    assert firm.mean() > 0.99
    return c, k, {"vtx_rotations": firm[:V], "uv_rotations": firm[V:]}


def _render(c, rast=None):
    """deform + forward of the scene -> (rasterizer, deformer, deformed dict, device camera tensors)."""
    from guava_renderer_amd.batch import BatchRasterizer
    P = c["V"] + c["N"]
    dfm = _deformer(c)
    cam = tuple(_t(c[n]) for n in ("views", "projs", "tanf", "bg"))
    rast = rast or BatchRasterizer(c["B"], P, W, W, R_capacity=64 * P * c["B"], device=DEV)
    verts, T = _t(c["verts"]), _t(c["vert_transforms"])
    d = dfm(verts, T)
    rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam)
    return rast, dfm, d, cam, verts, T


SEVEN = {"vtx_rotations": "vtx_rotations", "vtx_scales": "vtx_scales", "local_pos": "local_xyz",
         "uv_rotations": "uv_rotations", "uv_scales": "uv_scales", "colors": "colors", "opacity": "opacity"}


def _fused(c):
    rast, dfm, d, cam, verts, T = _render(c)
    g = rast.backward_deformed(dfm, verts, T, d, dfm.colors, dfm.opacity, *cam, _t(c["dL"]), _t(c["dLinv"]))
    torch.cuda.synchronize()
    assert not rast.status()[1] and not dfm.bad_index()
    radii = rast.radii.cpu().numpy()
    assert (radii > 0).any(0).mean() > 0.5  # the comparison is not of zeros
    assert radii[0, CULL_V] > 0 and radii[2, CULL_V] > 0 and radii[1, CULL_V] == 0  # culled in frame 1 only
    return {SEVEN[k]: v.cpu().numpy() for k, v in g.items()}, (rast, dfm, d, cam, verts, T)


def test_fused_backward_equals_composed():
    """backward_deformed vs BatchRasterizer.backward(shared=False) + gsr_deform_gaussians_backward on
    the same forward (render_bwd's atomics differ in the last bits run to run: the scale bar)."""
    c, k, masks = _scene()
    fused, (rast, dfm, d, cam, verts, T) = _fused(c)
    rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam)
    per = rast.backward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam, _t(c["dL"]),
                        _t(c["dLinv"]), shared=False)
    torch.cuda.synchronize()
    comp, bad = _gpu_backward(c, per["means3D"].cpu().numpy(), per["rotations"].cpu().numpy(),
                              per["scales"].cpu().numpy())
    assert bad == 0
    comp["colors"] = per["colors"].sum(0).cpu().numpy()
    comp["opacity"] = per["opacity"].sum(0).cpu().numpy()
    assert set(fused) == set(comp) and len(fused) == 7
    _compare("fused vs composed", fused, comp, masks)


def test_fused_backward_matches_float64_chain():
    """The per-frame oracle.backward gradients of the deformed attributes pushed through deform_ref's
    float64 autograd, colours and opacities summed over the frames."""
    import oracle
    c, k, masks = _scene()
    fused, (rast, dfm, d, cam, verts, T) = _fused(c)
    xyz, rot, scl = (d[n].cpu().numpy() for n in ("xyz", "rotation", "scaling"))
    B, P = c["B"], c["V"] + c["N"]
    g_xyz, g_rot, g_scl = np.zeros((B, P, 3)), np.zeros((B, P, 4)), np.zeros((B, P, 3))
    g_col, g_op = np.zeros((P, 32)), np.zeros((P, 1))
    for b, cm in enumerate(c["cams"]):
        a = (xyz[b], c["colors"], c["opacities"], scl[b], rot[b], None, cm["viewmatrix"], cm["projmatrix"], W, W,
             cm["tanfovx"], cm["tanfovy"], c["bg"][b])
        _, _, _, st = oracle.forward(*a)
        o = oracle.backward(st, *a, c["dL"][b], c["dLinv"][b][None])
        g_col += o[1]
        g_op += o[2]
        g_xyz[b], g_scl[b], g_rot[b] = o[3], o[6], o[7]
    ref = dict(zip(ATTRS, deform_ref.gradients(k, [c[a] for a in ATTRS], g_xyz, g_rot, g_scl)))
    ref["colors"], ref["opacity"] = g_col, g_op
    _compare("fused vs float64 chain", fused, ref, masks)


def _trainer(c, B, Wt, R_capacity):
    from guava_renderer_amd.train import AvatarTrainer
    V = c["V"]
    va = {"rotations": _t(c["vtx_rotations"]), "scales": _t(c["vtx_scales"]), "opacities": _t(c["opacities"][:V]),
          "colors": _t(c["colors"][:V])}
    ua = {"rotations": _t(c["uv_rotations"]), "scales": _t(c["uv_scales"]), "opacities": _t(c["opacities"][V:]),
          "colors": _t(c["colors"][V:]), "local_pos": _t(c["local_xyz"]), "binding_face": _t(c["binding_face"]),
          "face_bary": _t(c["face_bary"])}
    return AvatarTrainer(va, ua, _t(c["faces"]), B, Wt, Wt, R_capacity=R_capacity, device=DEV,
                         apply_rgb_sigmoid=False)


def test_trainer_gradients_are_the_fused_backward():
    from guava_renderer_amd.batch import BatchRasterizer
    c, k, masks = _scene()
    B, P = c["B"], c["V"] + c["N"]
    tr = _trainer(c, B, W, 64 * P * B)
    views, projs, tanf = _t(c["views"]), _t(c["projs"]), _t(c["tanf"])
    verts, T = _t(c["verts"]), _t(c["vert_transforms"])
    target = torch.rand((B, 3, W, W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    loss, grads = tr.gradients(verts, T, views, projs, tanf, target)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and set(grads) == set(tr.LEAVES)
    dL = tr._loss_bufs[1].clone()  # the image gradient that step's backward consumed
    dfm = _deformer(c)
    rast = BatchRasterizer(B, P, W, W, R_capacity=64 * P * B, device=DEV)
    d = dfm(verts, T)
    rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], views, projs, tanf, tr.bg)
    g = rast.backward_deformed(dfm, verts, T, d, dfm.colors, dfm.opacity, views, projs, tanf, tr.bg, dL, tr.dinv)
    torch.cuda.synchronize()
    g["opacities"] = g.pop("opacity")
    names = {"local_pos": "local_xyz"}
    _compare("trainer", {names.get(n, n): grads[n].cpu().numpy() for n in tr.LEAVES},
             {names.get(n, n): g[n].cpu().numpy() for n in tr.LEAVES}, masks)


def test_trainer_steps_lower_the_loss_and_skip_an_overflowing_step():
    from guava_renderer_amd import scenes
    from guava_renderer_amd.batch import BatchRasterizer
    c, k, masks = _scene()
    B, P, Wt = c["B"], c["V"] + c["N"], 64
    cams = scenes.frame_cameras(B, Wt, Wt, seed=5)
    views = _t(np.stack([cm["viewmatrix"].reshape(16) for cm in cams]))
    projs = _t(np.stack([cm["projmatrix"].reshape(16) for cm in cams]))
    tanf = _t(np.array([[cm["tanfovx"], cm["tanfovy"]] for cm in cams], np.float32))
    verts, T = _t(c["verts"]), _t(c["vert_transforms"])
    # targets: the same avatar rendered from perturbed attributes
    rng = np.random.default_rng(23)
    cp = dict(c)
    cp["colors"] = np.clip(c["colors"] + rng.normal(scale=0.2, size=c["colors"].shape), 0, 1).astype(np.float32)
    cp["uv_scales"] = (c["uv_scales"] * rng.uniform(0.7, 1.3, c["uv_scales"].shape)).astype(np.float32)
    cp["local_xyz"] = (c["local_xyz"] + rng.normal(scale=0.01, size=c["local_xyz"].shape)).astype(np.float32)
    dfm = _deformer(cp)
    rast = BatchRasterizer(B, P, Wt, Wt, R_capacity=64 * P * B, device=DEV)
    d = dfm(verts, T)
    col, _, _ = rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], views, projs, tanf,
                             torch.zeros((B, 32), device=DEV))
    target = col[:, :3].clone()
    tr = _trainer(c, B, Wt, 64 * P * B)
    losses = [tr.step(verts, T, views, projs, tanf, target).item() for _ in range(3)]
    torch.cuda.synchronize()
    print("  losses", losses)
    assert np.isfinite(losses).all() and losses[2] < losses[0]
    assert tr.skipped_steps == 0
    # a workspace too small for the batch: the step is skipped on the device, then the workspace grows
    tr2 = _trainer(c, B, Wt, 1000)
    before = {n: v.detach().clone() for n, v in tr2.p.items()}
    loss = tr2.step(verts, T, views, projs, tanf, target)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
    for n, v in tr2.p.items():
        assert torch.equal(v.detach(), before[n]), n
    with pytest.warns(UserWarning):
        loss2 = tr2.step(verts, T, views, projs, tanf, target)
    torch.cuda.synchronize()
    assert tr2.skipped_steps == 1 and tr2.rast.R_capacity > 1000 and torch.isfinite(loss2)
    assert any(not torch.equal(v.detach(), before[n]) for n, v in tr2.p.items())
