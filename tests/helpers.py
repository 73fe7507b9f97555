"""Shared test helpers: scene construction, GPU calls through the drop-in API, oracle calls and
scratch-arena decoding (mirrors carve_geom/carve_image/carve_bin in
guava_renderer_amd/csrc/capi.hip -- keep in sync)."""
import numpy as np

C = 32


def _align(x):
    return (x + 255) & ~255


def _carve(spec):
    off = 0
    out = {}
    for name, dtype, count in spec:
        off = _align(off)
        out[name] = (off, np.dtype(dtype), count)
        off += np.dtype(dtype).itemsize * count
    return out


def layout_bytes(layout):
    """Size of a carved arena (carve_*: the last slab's end, aligned, plus a 256-byte tail)."""
    return _align(max(off + dt.itemsize * count for off, dt, count in layout.values())) + 256


# gsr_internal.h: control words, per-frame words behind them, depth-sort sizes
CTRL_WORDS, FS_WORDS = 9216, 8
CTRL_NUM_BIG = 3
FS_NOT_KEY_MAX, FS_KEY_MAX, FS_VISIBLE = 0, 1, 2
TINY_BUCKET, SORT_SMALL_CAP, SORT_LARGE_CAP = 64, 2048, 8192


def _nb(P):
    """make_dims: depth buckets per frame, P / 16 up to 2^14 (2^20 above 512k Gaussians)."""
    cap = (1 << 14) if P <= (1 << 19) else (1 << 20)
    nb = 64
    while nb < P // 16 and nb < cap:
        nb <<= 1
    return nb


def geom_layout(P, W, H, B=1):
    """carve_geom of make_dims(B, P, W, H): per-frame slabs hold B frames back to back."""
    nblk = (P + 255) // 256
    T = ((W + 15) // 16) * ((H + 15) // 16)
    NB = _nb(P)
    chunk = 1024 if T > 1024 else 256  # make_dims: count-table rows
    nchunk = (P + chunk - 1) // chunk
    n = B * P
    return _carve([("ctrl", np.uint32, CTRL_WORDS + FS_WORDS * B), ("depth", np.float32, n),
                   ("invdepth", np.float32, n), ("radii", np.int32, n), ("means2D", np.float32, 2 * n),
                   ("cov3D", np.float32, 6 * n), ("conic", np.float32, 4 * n), ("rect", np.uint32, 2 * n),
                   ("rrec", np.float32, 8 * n), ("tiles", np.uint32, n), ("blocksums", np.uint32, B * nblk + 1),
                   ("blockkey", np.uint32, 2 * B * nblk), ("bslot", np.uint32, n),
                   ("bcount", np.uint32, B * (NB + 1)), ("bstart", np.uint32, B * (NB + 1)),
                   ("skey", np.uint64, n), ("big", np.uint32, B * NB), ("order", np.uint32, n),
                   ("table", np.uint32, B * nchunk * T), ("fsplit", np.uint32, P * C),
                   ("gterm", np.float32, 8 * n)])


def image_layout(W, H):
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return _carve([("final_T", np.float32, W * H), ("n_contrib", np.uint32, W * H),
                   ("ranges", np.uint32, 2 * T), ("tile_count", np.uint32, T), ("work_list", np.uint32, T),
                   ("lpt_hist", np.uint32, 34), ("strip_cnt", np.uint32, 4 * T),
                   ("strip_list", np.uint32, 4 * T), ("strip_hist", np.uint32, 8 * 129)])


def bin_layout(R):
    n = max(R, 1)
    return _carve([("point_list", np.uint32, n)])


def decode(buf_np, layout):
    out = {}
    for name, (off, dt, count) in layout.items():
        out[name] = np.frombuffer(buf_np[off:off + dt.itemsize * count].tobytes(), dtype=dt).copy()
    return out


def make_scene(kind="random", P=2000, W=128, H=96, seed=0, yaw=0.0, pitch=0.0):
    from guava_renderer_amd import camera, scenes
    if kind == "random":
        d = scenes.random_cloud(P, seed)
    else:
        d = scenes.avatar_cloud(P, seed)
    cam = camera.camera(W, H, yaw=yaw, pitch=pitch)
    d.update(cam)
    d["bg"] = np.zeros(C, np.float32)
    return d


def depth_cloud(P, seed, mode, levels=None, zspread=1.0, outliers=False, culled=0.0, small=1.0):
    """scenes.random_cloud with its z column rewritten to steer the per-frame depth sort.  With yaw 0
    the view rotation is the identity, so view depth is fl(z + camera distance): equal z gives equal
    depth bits.
      mode "plane":   every z = 0.125 -- one depth bucket holds every visible key, all tied
           "levels":  z drawn uniformly from `levels` (exact float32 values; repeat a value to weight
                      it) -- a few big all-tied buckets
           "squeeze": z * zspread
      outliers: Gaussian 0 at (0, -0.6, -15) with scale 1e-3 and Gaussian 1 at (0, -0.6, 68), both on
                the optical axis and in front of the camera for distances 20..25: they stretch the key
                range so the cloud falls into a few buckets of mostly distinct keys
      culled:   that fraction moved to x = 5 (off screen): V < P, and the order is not the identity
                on ties
      small:    scales multiplied by it (fewer instances, a quicker oracle)"""
    from guava_renderer_amd import scenes
    d = scenes.random_cloud(P, seed)
    rng = np.random.default_rng(seed + 7919)
    m = d["means3D"]
    if mode == "plane":
        m[:, 2] = np.float32(0.125)
    elif mode == "levels":
        m[:, 2] = np.asarray(levels, np.float32)[rng.integers(0, len(levels), P)]
    elif mode == "squeeze":
        m[:, 2] = (m[:, 2] * np.float32(zspread)).astype(np.float32)
    else:
        raise ValueError(mode)
    d["scales"] = (d["scales"] * np.float32(small)).astype(np.float32)
    if culled > 0.0:
        m[rng.random(P) < culled, 0] = np.float32(5.0)
    if outliers:
        m[0] = (0.0, -0.6, -15.0)
        d["scales"][0] = np.float32(1e-3)
        m[1] = (0.0, -0.6, 68.0)
    return d


def depth_scene(P, seed, mode, W=64, H=64, distance=22.0, **kw):
    """depth_cloud seen by the canonical camera (yaw 0) at `distance`, as make_scene returns it."""
    from guava_renderer_amd import camera
    d = depth_cloud(P, seed, mode, **kw)
    d.update(camera.camera(W, H, distance=distance))
    d["bg"] = np.zeros(C, np.float32)
    return d


def oracle_forward(d, exact=True, antialiasing=False, use_cov=False, scale_modifier=1.0):
    import oracle
    cov = None
    if use_cov:
        st = oracle.preprocess(d["means3D"], d["scales"], d["rotations"], d["opacities"], None,
                               d["viewmatrix"], d["projmatrix"], d["image_width"], d["image_height"],
                               d["tanfovx"], d["tanfovy"])
        cov = st["cov3D"]
    color, radii, invd, st = oracle.forward(
        d["means3D"], d["colors"], d["opacities"], None if use_cov else d["scales"],
        None if use_cov else d["rotations"], cov, d["viewmatrix"], d["projmatrix"],
        d["image_width"], d["image_height"], d["tanfovx"], d["tanfovy"], d["bg"],
        scale_modifier=scale_modifier, antialiasing=antialiasing, exact_exp=exact)
    return color, radii, invd, st


# Scenes that move the operands every other test holds at their trivial value (background, scale
# modifier, antialiasing) at small and ragged sizes: (id, kind, W, H, P, seed, xy factor, yaw, pitch,
# opacity override, scale_modifier, antialiasing).  tests/test_oracle.py pins the oracle on them
# against float64 autograd, tests/test_gpu_operands.py the GPU.
OPERAND_SCENES = (
    ("random48x32-mod0.6", "random", 48, 32, 40, 23, 0.25, 0.0, 0.0, None, 0.6, False),
    ("random48x32-mod1.7-aa", "random", 48, 32, 40, 23, 0.25, 0.0, 0.0, None, 1.7, True),
    ("random50x38-yaw-aa", "random", 50, 38, 150, 7, 0.15, 0.3, -0.2, None, 1.0, True),
    ("random17x33-saturated-mod1.3", "random", 17, 33, 120, 5, 0.1, 0.0, 0.0, 0.97, 1.3, False),
    ("avatar64x48-mod1.2-aa", "avatar", 64, 48, 400, 24, None, 0.0, 0.0, None, 1.2, True),
    ("random1x1", "random", 1, 1, 30, 9, 0.01, 0.0, 0.0, None, 1.0, False),
)


def operand_scene(row):
    """One row of OPERAND_SCENES -> (scene dict with a non-zero bg, dL[C,H,W], dLinv[1,H,W],
    scale_modifier, antialiasing)."""
    _, kind, W, H, P, seed, xy, yaw, pitch, opac, mod, aa = row
    d = make_scene(kind, P, W, H, seed=seed, yaw=yaw, pitch=pitch)
    if xy is not None:
        d["means3D"][:, :2] *= np.float32(xy)
    if opac is not None:
        d["opacities"][:] = np.float32(opac)
    rng = np.random.default_rng(3)
    d["bg"] = rng.uniform(-1.0, 2.0, C).astype(np.float32)
    dL = rng.normal(size=(C, H, W)).astype(np.float32)
    dLinv = rng.normal(size=(1, H, W)).astype(np.float32)
    return d, dL, dLinv, mod, aa


F64_NAMES = ("colors", "opacity", "means3D", "scales", "rotations", "means2D")


def float64_reference(d, st, dL=None, dLinv=None, scale_modifier=1.0, antialiasing=False):
    """tests/torch_ref.py on the scene, over the tile lists of the oracle state `st`: (image
    [C,H,W], n_contrib [H*W], gradients by F64_NAMES or None without dL), numpy float64.  "scales" is
    the gradient w.r.t. scale_modifier * scales and "means2D" the NDC one, as the reference returns
    them (torch_ref's docstring)."""
    import torch
    import torch_ref
    W, H = d["image_width"], d["image_height"]
    tile_lists = {t: st["point_list"][s:e] for t, (s, e) in enumerate(st["ranges"]) if e > s}
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    m3, sc, rot, op, colr = (f64(d["means3D"]), f64(d["scales"]), f64(d["rotations"]),
                              f64(d["opacities"].reshape(-1)), f64(d["colors"]))
    off = torch.zeros((m3.shape[0], 3), dtype=torch.float64, requires_grad=True)
    pr = torch_ref.project(m3, sc, rot, torch.tensor(d["viewmatrix"], dtype=torch.float64),
                           torch.tensor(d["projmatrix"], dtype=torch.float64), W, H, float(d["tanfovx"]),
                           float(d["tanfovy"]), scale_mod=float(scale_modifier), ndc_offset=off,
                           antialiasing=antialiasing)
    out, inv, _, nc = torch_ref.render(pr, op * pr["o1"], colr, torch.tensor(d["bg"], dtype=torch.float64),
                                       W, H, tile_lists)
    grads = None
    if dL is not None:
        loss = ((out * torch.tensor(dL, dtype=torch.float64)).sum()
                + (inv * torch.tensor(dLinv[0], dtype=torch.float64)).sum())
        loss.backward()
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731 (nothing rendered)
        grads = dict(colors=zero(colr), opacity=zero(op), means3D=zero(m3), scales=zero(pr["scales_eff"]),
                     rotations=zero(rot), means2D=zero(off)[:, :2])
        grads = {k: v.numpy() for k, v in grads.items()}
    return out.detach().numpy(), nc.numpy().reshape(-1), grads


def scale_err(a, ref):
    """max|a - ref| / max|ref|."""
    a = np.asarray(a, np.float64)
    ref = np.asarray(ref, np.float64)
    return float(np.abs(a.reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-30))


def torch_inputs(d, device="cuda", requires_grad=False):
    import torch
    t = {}
    for k in ("means3D", "colors", "opacities", "scales", "rotations"):
        t[k] = torch.tensor(d[k], device=device, requires_grad=requires_grad)
    t["viewmatrix"] = torch.tensor(d["viewmatrix"], device=device)
    t["projmatrix"] = torch.tensor(d["projmatrix"], device=device)
    t["campos"] = torch.tensor(d["campos"], device=device)
    t["bg"] = torch.tensor(d["bg"], device=device)
    return t


def gpu_forward(d, antialiasing=False, use_cov=None, debug=False, numerics=0, scale_modifier=1.0):
    """Runs _C.rasterize_gaussians; returns numpy outputs plus decoded scratch state."""
    import torch
    from guava_renderer_amd.diff_gaussian_rasterization_32 import _C
    t = torch_inputs(d)
    empty = torch.Tensor([])
    cov = empty if use_cov is None else torch.tensor(use_cov, device="cuda")
    scales = t["scales"] if use_cov is None else empty
    rots = t["rotations"] if use_cov is None else empty
    R, color, radii, gb, bb, ib, invd = _C.rasterize_gaussians(
        t["bg"], t["means3D"], t["colors"], t["opacities"], scales, rots, float(scale_modifier), cov,
        t["viewmatrix"], t["projmatrix"], d["tanfovx"], d["tanfovy"], d["image_height"],
        d["image_width"], empty, 0, t["campos"], False, antialiasing, debug, numerics=numerics)
    torch.cuda.synchronize()
    P = d["means3D"].shape[0]
    W, H = d["image_width"], d["image_height"]
    st = {}
    gl = geom_layout(P, W, H)
    assert layout_bytes(gl) == gb.numel(), ("geom_layout is out of step with carve_geom", layout_bytes(gl), gb.numel())
    st.update(decode(gb.cpu().numpy(), gl))
    st.update(decode(ib.cpu().numpy(), image_layout(W, H)))
    # the binning buffer is carved for its capacity: R after the synchronous read-back, the P x tiles
    # bound on the no-sync path
    from guava_renderer_amd import _lib
    L = _lib.load()
    cap = int(R) if bb.numel() == L.gsr_binning_bytes(int(R)) else L.gsr_forward_async_bound(P, W, H)
    st.update(decode(bb.cpu().numpy(), bin_layout(cap)))
    st["smask"] = st["point_list"] >> 28           # entries: index | strip mask << 28
    st["point_list"] = st["point_list"] & 0x0FFFFFFF
    st["R"] = R
    return color.cpu().numpy(), radii.cpu().numpy(), invd.cpu().numpy(), st


GRAD_SCALE_TOL = 1e-4   # |a - b| <= 1e-4 * max|b| over the whole tensor
GRAD_ELEM_TOL = 1e-3    # |a - b| <= 1e-3 * |b| on every element with |b| >= GRAD_ELEM_FLOOR * max|b|
GRAD_ELEM_FLOOR = 1e-3


NOISE_FACTOR = 1.5      # per-element bound relative to the reference algorithm's own f32 reordering noise
                        # (worst measured GPU / reordering ratio 1.26)


def grad_check(name, a, b, scale_tol=GRAD_SCALE_TOL, elem_tol=GRAD_ELEM_TOL, floor=GRAD_ELEM_FLOOR,
               noise=None, p999_tol=None):
    """Gradient parity, two ways: against the tensor's scale (the per-Gaussian atomics of the
    reference, backward.cu:593-635, reassociate freely) and per element -- a Gaussian with a small but
    not negligible gradient must be right too: relative error <= elem_tol on every element with
    |g| >= floor * max|g|.  `noise`: the same oracle gradient accumulated in another order
    (oracle.backward(reverse_order=True)); the closed-form backward amplifies f32 reassociation on
    ill-conditioned elements (the 2x2 conic inverse, computeCov2DCUDA, backward.cu:147-326), so the
    per-element bound is max(elem_tol, NOISE_FACTOR x the reference's own reordering error), and the
    99.9th percentile must stay within p999_tol (default elem_tol / 10).  Prints both distributions."""
    a = np.asarray(a, np.float64).reshape(-1)
    b = np.asarray(b, np.float64).reshape(-1)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    m = float(np.abs(b).max()) if b.size else 0.0
    if m == 0.0:
        assert np.abs(a).max(initial=0.0) == 0.0, name
        return
    err_scale = float(np.abs(a - b).max()) / m
    big = np.abs(b) >= floor * m
    rel = np.abs(a - b)[big] / np.abs(b)[big]
    p999 = float(np.percentile(rel, 99.9)) if rel.size else 0.0
    limit = elem_tol
    msg = ""
    if noise is not None:
        nz = np.asarray(noise, np.float64).reshape(-1)
        rel_n = np.abs(nz - b)[big] / np.abs(b)[big]
        limit = max(elem_tol, NOISE_FACTOR * float(rel_n.max(initial=0.0)))
        msg = (f"; reference reordered: max {rel_n.max(initial=0.0):.3g}, "
               f"p99.9 {float(np.percentile(rel_n, 99.9)) if rel_n.size else 0.0:.3g}")
    print(f"  {name}: {err_scale:.3g} of scale; elementwise over {int(big.sum())} |g| >= {floor:g} max: "
          f"max {rel.max(initial=0.0):.3g}, p99.9 {p999:.3g}{msg}")
    assert err_scale <= scale_tol, f"{name}: {err_scale:.3g} of scale"
    assert rel.max(initial=0.0) <= limit, f"{name}: element rel err {rel.max():.3g} > {limit:.3g} (p99.9 {p999:.3g})"
    p999_tol = elem_tol / 10 if p999_tol is None else p999_tol
    assert p999 <= p999_tol, f"{name}: element rel err p99.9 {p999:.3g} > {p999_tol:.3g}"
