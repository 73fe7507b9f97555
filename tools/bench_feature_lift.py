"""Feature lifting timings: the two projection gathers of the reference inferer at
512 x 512, U = 512, for B = 1 and B = 6 (config 4's batch per GPU) --
  uv        convert_pixel_feature_to_uv at C = 35 (RGB + 32 DINO channels), with the visibility term
  vertices  sample_prj_feature at C = 128 on the template's V = 10,475 vertices
-- forward alone (no_grad) and forward plus backward (autograd on the feature map), each against the
torch chain of the reference recipe (ubody_gaussian.py:75-114: einsums, gathers through the permuted
vertex tensor, grid_sample, isin / unique over the packed pix_to_face) on the same GPU tensors in the
same process.  The two sides alternate window by window; HIP events around each window of `--iters`
calls after a warm-up, median of `--repeats` windows.  The fused UV call takes MeshRasterizer's
face_visible [B,F]; the torch chain takes the packed pix_to_face, as the reference does.  Prints one
JSON line.

    python tools/bench_feature_lift.py [--iters 50] [--repeats 7] [--only uv:6]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def timed_pair(fa, fb, iters, repeats, warmup=5):
    """Medians (and ranges) of fa and fb, their windows alternating."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(repeats):
        a.append(window(fa, iters))
        b.append(window(fb, iters))
    s = lambda v: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}  # noqa: E731
    return s(a), s(b)


def torch_vertices(vertices, feature_map, w2c_cam, invtanfov):
    homo = torch.cat([vertices, torch.ones_like(vertices[:, :, :1])], dim=-1)
    cam = torch.einsum("bij,bnj->bni", w2c_cam, homo)[:, :, :3]
    img = cam * invtanfov / (cam[:, :, 2:] + 1e-7)
    s = torch.nn.functional.grid_sample(feature_map, img[:, None, :, :2], mode="bilinear", padding_mode="border",
                                        align_corners=False)
    return s.squeeze(-2).permute(0, 2, 1).contiguous(), img


def torch_uv(img_features, deformed_vertices, w2c_cam, invtanfov, faces, uvmap_f_idx, uvmap_f_bary, uvmap_mask,
             visble_faces):
    B = img_features.shape[0]
    bary = uvmap_f_bary[None].expand(B, -1, -1, -1)
    uv_vertex = deformed_vertices.permute(1, 2, 0).contiguous()[faces[uvmap_f_idx]]
    uv_vertex = uv_vertex.permute(4, 0, 1, 2, 3).contiguous()
    uv_vertex = torch.einsum("bhwk,bhwkn->bhwn", bary, uv_vertex)
    homo = torch.cat([uv_vertex, torch.ones_like(uv_vertex[:, :, :, :1])], dim=-1)
    cam = torch.einsum("bij,bhwj->bhwi", w2c_cam, homo)[:, :, :, :3]
    img = cam * invtanfov / (cam[..., 2:] + 1e-7)
    uv = torch.nn.functional.grid_sample(img_features, img[:, :, :, :2], mode="bilinear", padding_mode="zeros",
                                         align_corners=False)
    mask = uvmap_mask.clone()[None].repeat(B, 1, 1)
    F = faces.shape[0]
    off = torch.arange(B, device=faces.device, dtype=torch.int32) * F
    all_faces = torch.arange(0, F, device=faces.device, dtype=torch.int32)[None].repeat(B, 1) + off[:, None]
    mask = mask * torch.isin(all_faces, torch.unique(visble_faces))[:, uvmap_f_idx]
    return uv * mask[:, None]


def uv_layout(U, F, texel_count, seed=0):
    """75% of the texels placed, faces in order of the template's texels-per-face counts."""
    rng = np.random.default_rng(seed)
    face_of = np.repeat(np.arange(F), texel_count)
    n = U * U
    placed = np.sort(rng.choice(n, (3 * n) // 4, replace=False))
    f_idx = np.zeros(n, np.int64)
    f_idx[placed] = face_of[(np.arange(placed.size) * face_of.size) // placed.size]
    mask = np.zeros(n, np.float32)
    mask[placed] = 1.0
    bary = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    return f_idx.reshape(U, U), bary.reshape(U, U, 3), mask.reshape(U, U)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--only", default=None, help="one case, e.g. uv:6 or vertices:1")
    a = ap.parse_args()
    from guava_renderer_amd import avatar, camera
    from guava_renderer_amd.feature_lift import FeatureLifter
    from guava_renderer_amd.mesh_raster import BaseMeshRenderer
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = "cuda:0"
    verts, faces, texel_count = avatar.template_mesh()
    V, F, S = verts.shape[0], faces.shape[0], a.size
    U = S
    f_idx, f_bary, mask = uv_layout(U, F, texel_count)
    lifter = FeatureLifter(faces, f_idx, f_bary, mask, image_size=S, focal_length=24, device=dev)
    t_faces = torch.from_numpy(faces.astype(np.int64)).to(dev)
    t_idx, t_bary, t_mask = torch.from_numpy(f_idx).to(dev), torch.from_numpy(f_bary).to(dev), torch.from_numpy(mask).to(dev)
    out = {"workload": "feature lifting, SMPL-X template", "V": V, "F": F, "W": S, "H": S, "U": U, "iters": a.iters,
           "repeats": a.repeats, "cases": []}
    rng = np.random.default_rng(0)
    for name, B, C in (("uv", 1, 35), ("uv", 6, 35), ("vertices", 1, 128), ("vertices", 6, 128)):
        if a.only and a.only != f"{name}:{B}":
            continue
        w2c = torch.from_numpy(np.stack([camera.look_at_w2c(2 * np.pi * b / max(B, 6), 0.1, 22.0)
                                         for b in range(B)]).astype(np.float32)).to(dev)
        dv = torch.from_numpy(np.stack([verts + rng.normal(0, 0.002, 3).astype(np.float32) for _ in range(B)])).to(dev)
        feat = torch.randn((B, C, S, S), device=dev)
        fg = feat.clone().requires_grad_(True)
        if name == "uv":
            rend = BaseMeshRenderer(faces, image_size=S, focal_length=24, max_batch=B, device=dev)
            packed, _ = rend.render_fragments(dv, transform_matrix=w2c)
            vis = rend.rasterizer(dv, w2c, rend.tanfovx, rend.tanfovy).face_visible
            dout = torch.randn((B, C, U, U), device=dev)
            ours = lambda f: lifter.convert_pixel_feature_to_uv(f, dv, w2c, face_visible=vis)  # noqa: E731
            ref = lambda f: torch_uv(f, dv, w2c, 24.0, t_faces, t_idx, t_bary, t_mask, packed)  # noqa: E731
            live = int((ours(torch.ones_like(feat))[:, 0] != 0).sum())
            n_out = B * C * U * U
            geom = U * U * 16 + B * V * 12 + F * 12 + B * F
        else:
            dout = torch.randn((B, V, C), device=dev)
            ours = lambda f: lifter.sample_prj_feature(dv, f, w2c)[0]  # noqa: E731
            ref = lambda f: torch_vertices(dv, f, w2c, 24.0)[0]  # noqa: E731
            live = B * V
            n_out = B * V * C
            geom = B * V * 12
        err = float((ours(feat) - ref(feat)).abs().max())

        def fwd(fn):
            def run():
                with torch.no_grad():
                    fn(feat)
            return run

        def fwd_bwd(fn):
            def run():
                fg.grad = None
                fn(fg).backward(dout)
            return run
        f_o, f_t = timed_pair(fwd(ours), fwd(ref), a.iters, a.repeats)
        b_o, b_t = timed_pair(fwd_bwd(ours), fwd_bwd(ref), a.iters, a.repeats)
        n_map = B * C * S * S
        taps = live * 4 * C
        fwd_bytes = 4 * (min(taps, n_map) + n_out) + geom
        bwd_bytes = 4 * (n_out + n_map) + geom  # dout read, dfeat written
        atomic_bytes = 4 * taps
        bwd_us = max(b_o["median"] - f_o["median"], 1e-3)
        out["cases"].append({
            "case": name, "B": B, "C": C, "live_samples": live, "max_abs_diff_vs_torch": err,
            "forward_us": f_o, "torch_forward_us": f_t, "forward_speedup": round(f_t["median"] / f_o["median"], 2),
            "forward_backward_us": b_o, "torch_forward_backward_us": b_t,
            "forward_backward_speedup": round(b_t["median"] / b_o["median"], 2),
            "forward_algorithmic_bytes": fwd_bytes, "forward_GBs_algorithmic": round(fwd_bytes / f_o["median"] / 1e3, 1),
            "backward_algorithmic_bytes": bwd_bytes, "backward_scratch_bytes": 8 * n_map,
            "backward_atomic_bytes": atomic_bytes, "backward_us_by_difference": round(bwd_us, 1),
            "backward_GBs_algorithmic": round(bwd_bytes / bwd_us / 1e3, 1),
            "backward_atomic_GBs": round(atomic_bytes / bwd_us / 1e3, 1)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
