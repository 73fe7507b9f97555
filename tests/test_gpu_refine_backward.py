"""GPU tests of the differentiable fused refiner head (include/gsr.h gsr_refine_backward_*,
BatchRasterizer.backward_refine / backward_deformed(refine=), batch.render_refined).

With M the 32x32 map of gsr_refine_prepare (identity on [0, keep), the conv weight on
[keep, keep + n_out), zero below), the refine forward composites f' = M f, so its backward is the
ordinary batch backward on the prepared rows between an image end (the gradient image in prepared
channel space G', plus dbias and S = sum_px final_T dz) and a row end (dL/df = M^T d', dW).

Bars:
 * the row kernel alone against float64 from the same d': |err| <= n 2^-24 sum|terms| per element
   of dW (n rows: the plain f32 accumulation bound), n_out 2^-24 sum|terms| per element of dL/df;
 * the image kernel alone: G' bit-exact (one multiply per element), the sums within
   N_px 2^-24 sum|terms|;
 * end to end against the CPU oracle on the RAW colours with dL_dpix = M^T G' (float64 from the fused
   forward's own sign mask, cast to f32): attribute gradients through helpers.grad_check at its
   defaults, dW and dbias at GRAD_SCALE_TOL.
   Measured on MI355X: dW 2.5e-7 of scale and dbias 9.5e-8 (B = 3, P = 6000, 96 x 80), dW 1.4e-7 and
   dbias 1.7e-7 (B = 1, P = 2000, 64 x 64), per frame and frame-reduced alike: both hold
   GRAD_SCALE_TOL, so no wider bar was needed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import GRAD_SCALE_TOL, geom_layout, grad_check, layout_bytes, scale_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _head(n_out=16, keep=4, seed=1, bias=True):
    from guava_renderer_amd.batch import RefineHead
    rng = np.random.default_rng(seed)
    w = rng.normal(0, 0.2, (n_out, 32)).astype(np.float32)
    b = rng.normal(0, 0.1, n_out).astype(np.float32)
    return RefineHead(_t(w), _t(b) if bias else None, keep_channels=keep)


# ------------------------------------------------------------------------------- the row kernel alone

ROW_COUNTS = (1, 2, 3, 63, 64, 65, 257, 4097)  # 257: one row past a workgroup's 256; 4097: 17 workgroups


def _rows_call(n, frames, dp, raw, raw_stride, B, sums, bg, head_w, n_out, keep):
    """gsr_refine_backward_rows through ctypes -> (rows, dW, dbias) tensors."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    nbytes = L.gsr_refine_backward_scratch_bytes(B, 1, 1, n, frames)
    scratch = torch.zeros(nbytes // 4, dtype=torch.float32, device=DEV)
    scratch[:B * 64] = sums.reshape(-1)
    rows = torch.full_like(dp, float("nan"))
    dW = torch.full((n_out, 32), float("nan"), device=DEV)
    db = torch.full((n_out,), float("nan"), device=DEV)
    desc = _lib.RefineBackwardDesc(head_w.data_ptr(), n_out, keep, 0.2, 0, None, None, None, None, scratch.data_ptr())
    rc = L.gsr_refine_backward_rows(n, frames, dp.data_ptr(), raw.data_ptr(), raw_stride, B, scratch.data_ptr(),
                                    bg.data_ptr(), 32, ctypes.byref(desc), rows.data_ptr(), dW.data_ptr(),
                                    db.data_ptr(), _stream())
    _lib.check(rc, "gsr_refine_backward_rows")
    torch.cuda.synchronize()
    return rows, dW, db


@pytest.mark.parametrize("mode", ["reduced", "per_frame", "shared"])
@pytest.mark.parametrize("n_out,keep", [(16, 4), (3, 0), (28, 4), (1, 31)])
def test_row_kernel_matches_float64(n_out, keep, mode):
    """reduced: one frame of rows (the frame-reduced d'); per_frame: B = 3 frames of rows, each with
    its own raw rows; shared: B = 3 frames of rows over one raw table (stride 0)."""
    B = 3
    frames = 1 if mode == "reduced" else B
    rng = np.random.default_rng(100 * n_out + keep)
    W = rng.normal(0, 0.3, (n_out, 32)).astype(np.float32)
    bg = rng.normal(size=(B, 32)).astype(np.float32)
    sums = rng.normal(size=(B, 64)).astype(np.float32)
    for n in ROW_COUNTS:
        dp = rng.normal(size=(frames, n, 32)).astype(np.float32)  # (channels past keep + n_out are ignored)
        raw = rng.normal(size=(frames if mode == "per_frame" else 1, n, 32)).astype(np.float32)
        stride = n * 32 if mode == "per_frame" else 0
        f64 = np.broadcast_to(raw.astype(np.float64), (frames, n, 32))
        d64 = dp.astype(np.float64)
        dz = d64[:, :, keep:keep + n_out]
        dW_rows = np.einsum("fro,frc->oc", dz, f64)
        dW_abs = np.einsum("fro,frc->oc", np.abs(dz), np.abs(f64))
        W64 = W.astype(np.float64)
        df_ref = np.einsum("fro,oc->frc", dz, W64)
        df_abs = np.einsum("fro,oc->frc", np.abs(dz), np.abs(W64))
        df_ref[:, :, :keep] += d64[:, :, :keep]
        df_abs[:, :, :keep] += np.abs(d64[:, :, :keep])
        for with_sums in (False, True):
            s = sums if with_sums else np.zeros_like(sums)
            got = _rows_call(frames * n, frames, _t(dp), _t(raw), stride, B, _t(s), _t(bg), _t(W), n_out, keep)
            rows, dW, db = (x.cpu().numpy().astype(np.float64) for x in got)
            s64 = s.astype(np.float64)
            sbg = np.einsum("bo,bc->oc", s64[:, 32:32 + n_out], bg.astype(np.float64))
            sbg_abs = np.einsum("bo,bc->oc", np.abs(s64[:, 32:32 + n_out]), np.abs(bg.astype(np.float64)))
            # n rows: the plain f32 accumulation bound; the B background terms extend the same chain
            terms = frames * n + (B if with_sums else 0)
            bound = terms * U * (dW_abs + sbg_abs)
            err = np.abs(dW - (dW_rows + sbg))
            assert np.isfinite(dW).all() and (err <= bound).all(), \
                (n, with_sums, float((err / np.maximum(bound, 1e-300)).max()))
            db_ref = s64[:, :n_out].sum(0)
            assert (np.abs(db - db_ref) <= B * U * np.abs(s64[:, :n_out]).sum(0)).all(), (n, with_sums)
            err = np.abs(rows - df_ref)
            assert np.isfinite(rows).all() and (err <= n_out * U * df_abs).all(), \
                (n, float((err / np.maximum(n_out * U * df_abs, 1e-300)).max()))
            again = _rows_call(frames * n, frames, _t(dp), _t(raw), stride, B, _t(s), _t(bg), _t(W), n_out, keep)
            for a, b in zip(got, again):
                assert torch.equal(a, b), (n, "not reproducible")


# ----------------------------------------------------------------------------- the image kernel alone

@pytest.mark.parametrize("with_keep", [True, False])
def test_image_kernel_bit_exact_and_deterministic(with_keep):
    from guava_renderer_amd import _lib, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    L = _lib.load()
    B, P, W, H, n_out, keep, slope = 2, 500, 50, 37, 16, 4, 0.2
    sc = scenes.random_cloud(P, seed=5)
    cams = scenes.frame_cameras(B, W, H, seed=9)
    views = _t(np.stack([c["viewmatrix"].reshape(16) for c in cams]))
    projs = _t(np.stack([c["projmatrix"].reshape(16) for c in cams]))
    tanf = _t(np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32))
    r = BatchRasterizer(B, P, W, H, device=DEV)
    r.forward(*[_t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")], views, projs, tanf,
              torch.zeros((B, 32), device=DEV))
    torch.cuda.synchronize()
    assert not r.status()[1]
    gsz = layout_bytes(geom_layout(P, W, H, B))
    T = r.workspace[gsz:gsz + 4 * B * H * W].view(torch.float32).cpu().numpy().reshape(B, H * W)
    assert T.min() >= 0.0 and T.max() <= 1.0 and (T < 1.0).any() and np.unique(T).size > 100  # a real render
    rng = np.random.default_rng(6)
    out = rng.normal(size=(B, n_out, H, W)).astype(np.float32)
    flat = out.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    assert (np.signbit(flat) & (flat == 0)).any() and ((flat == 0) & ~np.signbit(flat)).any()
    dout = rng.normal(size=(B, n_out, H, W)).astype(np.float32)
    dkeep = rng.normal(size=(B, keep, H, W)).astype(np.float32)
    w = _t(rng.normal(size=(n_out, 32)).astype(np.float32))
    t_out, t_dout, t_dkeep = _t(out), _t(dout), _t(dkeep)
    nbytes = L.gsr_refine_backward_scratch_bytes(B, W, H, P, 1)

    def run():
        G = torch.full((B, 32, H, W), float("nan"), device=DEV)
        scratch = torch.full((nbytes // 4,), float("nan"), device=DEV)
        desc = _lib.RefineBackwardDesc(w.data_ptr(), n_out, keep, slope, 0, t_out.data_ptr(), t_dout.data_ptr(),
                                       t_dkeep.data_ptr() if with_keep else None, G.data_ptr(), scratch.data_ptr())
        _lib.check(L.gsr_refine_backward_image(B, P, W, H, r.workspace.data_ptr(), r.R_capacity, ctypes.byref(desc),
                                               _stream()), "gsr_refine_backward_image")
        torch.cuda.synchronize()
        return G, scratch[:B * 64].clone()
    G, sums = run()
    dz = dout * np.where(out > 0, np.float32(1.0), np.float32(slope)).astype(np.float32)
    ref = np.zeros((B, 32, H, W), np.float32)
    if with_keep:
        ref[:, :keep] = dkeep
    ref[:, keep:keep + n_out] = dz
    g = G.cpu().numpy()
    assert np.array_equal(g.view(np.uint32), ref.view(np.uint32))  # all 32 channels, bit for bit (incl. -0)
    assert not g[:, keep + n_out:].any()
    s = sums.cpu().numpy().astype(np.float64).reshape(B, 64)
    dz64 = dz.astype(np.float64).reshape(B, n_out, H * W)
    npx = H * W
    db_ref, db_abs = dz64.sum(2), np.abs(dz64).sum(2)
    S_ref = (dz64 * T[:, None].astype(np.float64)).sum(2)
    S_abs = np.abs(dz64 * T[:, None]).sum(2)
    assert (np.abs(s[:, :n_out] - db_ref) <= npx * U * db_abs).all()
    assert (np.abs(s[:, 32:32 + n_out] - S_ref) <= npx * U * S_abs).all()
    assert not s[:, n_out:32].any() and not s[:, 32 + n_out:].any()
    G2, sums2 = run()
    assert torch.equal(G, G2) and torch.equal(sums, sums2)


def test_forward_only_workspace_is_refused():
    from guava_renderer_amd import _lib, scenes
    from guava_renderer_amd.batch import BatchRasterizer
    L = _lib.load()
    B, P, W, H = 1, 300, 32, 32
    sc = scenes.random_cloud(P, seed=2)
    cam = scenes.frame_cameras(2, W, H, seed=1)[0]
    head = _head()
    r = BatchRasterizer(B, P, W, H, device=DEV)
    r.forward(*[_t(sc[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")],
              _t(cam["viewmatrix"].reshape(1, 16)), _t(cam["projmatrix"].reshape(1, 16)),
              _t(np.array([[cam["tanfovx"], cam["tanfovy"]]], np.float32)), torch.zeros(32, device=DEV),
              refine=head, forward_only=True)
    with pytest.raises(_lib.GsrError):
        r.refine_backward_image(head, torch.zeros_like(head.out))
    G = torch.zeros((B, 32, H, W), device=DEV)
    scratch = torch.zeros(L.gsr_refine_backward_scratch_bytes(B, W, H, P, 1) // 4, device=DEV)
    dout = torch.zeros_like(head.out)
    desc = _lib.RefineBackwardDesc(head.weight.data_ptr(), 16, 4, 0.2, 0, head.out.data_ptr(), dout.data_ptr(), None,
                                   G.data_ptr(), scratch.data_ptr())
    rc = L.gsr_refine_backward_image(B, P, W, H, r.workspace.data_ptr(), r.R_capacity, ctypes.byref(desc), _stream())
    assert rc == -1 and b"GSR_FORWARD_ONLY" in L.gsr_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ end to end

ATTRS = ("means3D", "colors", "opacities", "scales", "rotations")
# gradient name in backward()'s dict -> index in oracle.backward's tuple
ORACLE_IDX = {"means3D": 3, "colors": 1, "opacity": 2, "scales": 6, "rotations": 7}


@functools.lru_cache(maxsize=None)
def _e2e_scene(B, P, W, H):
    from guava_renderer_amd import scenes
    sc = scenes.random_cloud(P, seed=3)
    cams = scenes.frame_cameras(max(B, 2), W, H, seed=7)[:B]
    rng = np.random.default_rng(0)
    return dict(sc=sc, cams=cams, bgs=rng.normal(size=(B, 32)).astype(np.float32),
                views=np.stack([c["viewmatrix"].reshape(16) for c in cams]),
                projs=np.stack([c["projmatrix"].reshape(16) for c in cams]),
                tanf=np.array([[c["tanfovx"], c["tanfovy"]] for c in cams], np.float32),
                dLr=rng.normal(size=(B, 16, H, W)).astype(np.float32),
                dLraw=rng.normal(size=(B, 4, H, W)).astype(np.float32),
                dLinv=rng.normal(size=(B, H, W)).astype(np.float32))


def _gpu_args(s):
    return tuple(_t(s["sc"][k]) for k in ATTRS) + (_t(s["views"]), _t(s["projs"]), _t(s["tanf"]), _t(s["bgs"]))


@functools.lru_cache(maxsize=None)
def _e2e_reference(B, P, W, H):
    """(fused forward's refined output, per-frame oracle gradients, their reverse-order twins, dW and
    dbias in float64): the oracle runs on the RAW colours and backgrounds with dL_dpix = M^T G', G' from
    the fused forward's own sign mask.  Computed once, never modified."""
    import oracle
    from guava_renderer_amd.batch import BatchRasterizer
    s = _e2e_scene(B, P, W, H)
    head = _head()
    r = BatchRasterizer(B, P, W, H, device=DEV)
    r.forward(*_gpu_args(s), refine=head)
    torch.cuda.synchronize()
    assert not r.status()[1]
    out = head.out.cpu().numpy()
    W64 = head.weight.cpu().numpy().astype(np.float64)
    dz = s["dLr"].astype(np.float64) * np.where(out > 0, 1.0, np.float64(np.float32(head.slope)))
    dpix = np.einsum("bohw,oc->bchw", dz, W64)
    dpix[:, :4] += s["dLraw"]
    dpix = dpix.astype(np.float32)
    sc = s["sc"]
    fwd, rev = [], []
    dW, db = np.zeros((16, 32)), dz.sum((0, 2, 3))
    for f, c in enumerate(s["cams"]):
        a = (sc["means3D"], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"], None, c["viewmatrix"],
             c["projmatrix"], W, H, c["tanfovx"], c["tanfovy"], s["bgs"][f])
        img, _, _, st = oracle.forward(*a)
        fwd.append(oracle.backward(st, *a, dpix[f], s["dLinv"][f][None]))
        rev.append(oracle.backward(st, *a, dpix[f], s["dLinv"][f][None], reverse_order=True))
        dW += np.einsum("ohw,chw->oc", dz[f], img.astype(np.float64))
    return fwd, rev, dW, db


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,P,W,H", [(3, 6000, 96, 80), (1, 2000, 64, 64)])
def test_backward_refine_matches_oracle(B, P, W, H, shared):
    """B = 3: test_refine_epilogue_matches_conv's scene (ragged image, per-frame backgrounds, bias,
    16/4); B = 1: the single-frame refine kernel's final_T."""
    from guava_renderer_amd.batch import BatchRasterizer
    s = _e2e_scene(B, P, W, H)
    fwd, rev, dW_ref, db_ref = _e2e_reference(B, P, W, H)
    head = _head()
    r = BatchRasterizer(B, P, W, H, device=DEV)
    args = _gpu_args(s)
    r.forward(*args, refine=head)
    g = r.backward_refine(head, *args, _t(s["dLr"]), dL_draw=_t(s["dLraw"]), dL_dinvdepth=_t(s["dLinv"]),
                          shared=shared)
    torch.cuda.synchronize()
    assert not r.status()[1]
    for name, idx in ORACLE_IDX.items():
        mine = g[name].cpu().numpy()
        if shared:
            assert mine.shape[0] == P
            grad_check(f"shared {name}", mine, sum(np.asarray(o[idx], np.float64) for o in fwd),
                       noise=sum(np.asarray(o[idx], np.float64) for o in rev))
        else:
            for f in range(B):
                grad_check(f"frame {f} {name}", mine[f], fwd[f][idx], noise=rev[f][idx])
    eW, eb = scale_err(g["weight"].cpu().numpy(), dW_ref), scale_err(g["bias"].cpu().numpy(), db_ref)
    print(f"  dW {eW:.3g} of scale, dbias {eb:.3g} of scale (shared={shared})")
    assert eW <= GRAD_SCALE_TOL and eb <= GRAD_SCALE_TOL, (eW, eb)


# -------------------------------------------------------------------------------------------- autograd

def test_render_refined_autograd_matches_backward_refine():
    from guava_renderer_amd import _lib
    from guava_renderer_amd.batch import BatchRasterizer, render_refined
    B, P, W, H = 3, 6000, 96, 80
    s = _e2e_scene(B, P, W, H)
    args = _gpu_args(s)
    head = _head()
    r = BatchRasterizer(B, P, W, H, device=DEV)
    leaves = [a.clone().requires_grad_(True) for a in args[:5]]
    w = head.weight.clone().reshape(16, 32, 1, 1).requires_grad_(True)
    b = head.bias.clone().requires_grad_(True)
    raw, refined, invd, radii = render_refined(r, w, b, *leaves, *args[5:])
    assert raw.shape == (B, 4, H, W) and refined.shape == (B, 16, H, W) and invd.shape == (B, H, W)
    assert radii.shape == (B, P) and not radii.requires_grad
    g1, g2, g3 = _t(s["dLr"]), _t(s["dLraw"]), _t(s["dLinv"])
    ((refined * g1).sum() + (raw * g2).sum() + (invd * g3).sum()).backward()
    r.forward(*args, refine=head)
    assert torch.equal(head.out, refined) and torch.equal(r.out_color[:, :4], raw)
    ref = r.backward_refine(head, *args, g1, dL_draw=g2, dL_dinvdepth=g3, shared=True)
    torch.cuda.synchronize()
    for leaf, name in zip(leaves, ("means3D", "colors", "opacity", "scales", "rotations")):
        e = scale_err(leaf.grad.cpu().numpy(), ref[name].cpu().numpy())
        print(f"  autograd {name}: {e:.3g} of scale")
        assert leaf.grad.shape == leaf.shape and e <= GRAD_SCALE_TOL, (name, e)
    assert w.grad.shape == w.shape
    assert scale_err(w.grad.reshape(16, 32).cpu().numpy(), ref["weight"].cpu().numpy()) <= GRAD_SCALE_TOL
    assert scale_err(b.grad.cpu().numpy(), ref["bias"].cpu().numpy()) <= GRAD_SCALE_TOL
    # `refined` is the call's own tensor: a later forward leaves it alone; and that later forward makes
    # the first call's backward an error instead of the wrong frame's gradients
    raw_a, refined_a, _, _ = render_refined(r, w, b, *leaves, *args[5:])
    keep = refined_a.detach().clone()
    bgs2 = args[8] + 1.0
    raw_b, refined_b, _, _ = render_refined(r, w, b, *leaves, *args[5:8], bgs2)
    torch.cuda.synchronize()
    assert torch.equal(refined_a.detach(), keep) and not torch.equal(refined_b.detach(), keep)
    with pytest.raises(_lib.GsrError, match="another forward"):
        refined_a.sum().backward()
    refined_b.sum().backward()  # the latest forward's backward still runs
    torch.cuda.synchronize()


def test_render_refined_per_frame_attributes_sum_the_shared_ones():
    """Per-frame colours [B,P,32] beside shared geometry: the per-frame backward, the shared leaves
    getting the sum over the frames."""
    from guava_renderer_amd.batch import BatchRasterizer, render_refined
    B, P, W, H = 3, 6000, 96, 80
    s = _e2e_scene(B, P, W, H)
    args = _gpu_args(s)
    head = _head()
    r = BatchRasterizer(B, P, W, H, device=DEV)
    leaves = [a.clone().requires_grad_(True) for a in args[:5]]
    leaves[1] = args[1][None].repeat(B, 1, 1).requires_grad_(True)
    w, b = head.weight.clone().requires_grad_(True), head.bias.clone().requires_grad_(True)
    raw, refined, invd, _ = render_refined(r, w, b, *leaves, *args[5:])
    g1, g2 = _t(s["dLr"]), _t(s["dLraw"])
    ((refined * g1).sum() + (raw * g2).sum()).backward()
    r.forward(*args, refine=head)
    ref = r.backward_refine(head, *args, g1, dL_draw=g2, shared=False)
    torch.cuda.synchronize()
    assert leaves[1].grad.shape == (B, P, 32)
    assert scale_err(leaves[1].grad.cpu().numpy(), ref["colors"].cpu().numpy()) <= GRAD_SCALE_TOL
    for leaf, name in ((leaves[0], "means3D"), (leaves[2], "opacity"), (leaves[3], "scales"), (leaves[4], "rotations")):
        assert scale_err(leaf.grad.cpu().numpy(), ref[name].sum(0).cpu().numpy()) <= GRAD_SCALE_TOL, name
    assert scale_err(w.grad.cpu().numpy(), ref["weight"].cpu().numpy()) <= GRAD_SCALE_TOL


# -------------------------------------------------------------------------------------------- overflow

def test_overflowed_forward_has_zero_gradients():
    from guava_renderer_amd import _lib
    from guava_renderer_amd.batch import BatchRasterizer
    B, P, W, H = 2, 2000, 64, 64
    s = _e2e_scene(B, P, W, H)
    args = _gpu_args(s)
    head = _head()
    r = BatchRasterizer(B, P, W, H, R_capacity=16, device=DEV)
    col, inv, _ = r.forward(*args, refine=head)
    assert torch.isnan(head.out).all() and torch.isnan(col[:, :4]).all()
    g = r.backward_refine(head, *args, _t(s["dLr"]), dL_draw=_t(s["dLraw"]), dL_dinvdepth=_t(s["dLinv"]), shared=True)
    torch.cuda.synchronize()
    assert set(g) >= {"means3D", "colors", "opacity", "scales", "rotations", "weight", "bias"}
    for k, v in g.items():
        assert not torch.isnan(v).any() and not v.any(), k
    with pytest.raises(_lib.CapacityError):
        r.poll(wait=True)


# ---------------------------------------------------------------------------------------- posed avatar

def test_backward_deformed_refine_equals_the_composition():
    """backward_deformed(refine=head, dL_drefined=) on test_gpu_deform_backward's rendered avatar
    (96 x 96, B = 3) against the three steps called by hand."""
    from guava_renderer_amd.batch import BatchRasterizer
    from test_gpu_deform_backward import W as WA, _deformer, _scene
    c, _, _ = _scene()
    B, P = c["B"], c["V"] + c["N"]
    head = _head(seed=4)
    dfm = _deformer(c)
    cam = tuple(_t(c[n]) for n in ("views", "projs", "tanf", "bg"))
    rast = BatchRasterizer(B, P, WA, WA, R_capacity=64 * P * B, device=DEV)
    verts, T = _t(c["verts"]), _t(c["vert_transforms"])
    d = dfm(verts, T)
    rast.forward(d["xyz"], dfm.colors, dfm.opacity, d["scaling"], d["rotation"], *cam, refine=head)
    rng = np.random.default_rng(31)
    dLr = _t(rng.normal(size=(B, 16, WA, WA)).astype(np.float32))
    dLraw = _t(rng.normal(size=(B, 4, WA, WA)).astype(np.float32))
    dLinv = _t(c["dLinv"])
    fused = rast.backward_deformed(dfm, verts, T, d, dfm.colors, dfm.opacity, *cam, dL_dinvdepth=dLinv, refine=head,
                                   dL_drefined=dLr, dL_draw=dLraw)
    G, scratch = rast.refine_backward_image(head, dLr, dLraw)
    raw = dfm.colors if dfm.colors.dim() == 2 else dfm.colors[0]
    pc = head.prepare(raw.contiguous(), _stream(), cache=False)
    pb = head.prepare(cam[3].contiguous(), _stream(), cache=False)
    mid = rast.backward_deformed(dfm, verts, T, d, pc, dfm.opacity, cam[0], cam[1], cam[2], pb, G, dLinv)
    rows, dW, db = rast.refine_backward_rows(head, mid["colors"], raw, cam[3], scratch)
    torch.cuda.synchronize()
    assert not rast.status()[1] and (rast.radii > 0).any(0).float().mean() > 0.5
    assert set(fused) == set(mid) | {"weight", "bias"}
    hand = dict(mid, colors=rows, weight=dW, bias=db)
    for k in ("colors", "opacity", "vtx_rotations", "vtx_scales", "local_pos", "uv_rotations", "uv_scales", "weight",
              "bias"):
        e = scale_err(fused[k].cpu().numpy(), hand[k].cpu().numpy())
        print(f"  fused vs by hand {k}: {e:.3g} of scale")
        assert fused[k].abs().max() > 0 and e <= GRAD_SCALE_TOL, (k, e)
