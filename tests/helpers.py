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
CTRL_R, CTRL_NUM_BIG, CTRL_NON_EMPTY, CTRL_QSTART = 0, 3, 6, 16
FS_NOT_KEY_MAX, FS_KEY_MAX, FS_VISIBLE, FS_R, FS_RBASE, FS_NON_EMPTY = 0, 1, 2, 3, 4, 5
TINY_BUCKET, SORT_SMALL_CAP, SORT_LARGE_CAP = 64, 2048, 8192
SLOTS = 256                     # kSlots: Gaussians per ordered-scatter pass
LPT_BUCKETS, STRIP_BUCKETS = 34, 129
INDEX_MASK = (1 << 28) - 1      # kIndexMask: point_list entry -> Gaussian index; the strip mask sits above
MAX_TILES = 16384               # kMaxTiles


def tile_queue(t, gx):
    """gsr_internal.h tile_queue: the XCD queue of tile t of a frame (4x4-tile blocks, shifted by 3 per
    block row).  Scalars or arrays."""
    tx, ty = t % gx, t // gx
    return ((tx >> 2) + 3 * (ty >> 2)) & 7


def strip_bucket(c):
    """binning.hip strip_bucket: 4 buckets per octave of survivors, most first; 128 = none."""
    c = int(c)
    if c == 0:
        return STRIP_BUCKETS - 1
    e = c.bit_length() - 1
    sub = (c >> (e - 2)) & 3 if e >= 2 else (c << (2 - e)) & 3
    return 127 - (4 * e + sub)


def lpt_bucket(c):
    """k_tile_scan's work-list bucket of a tile with c list entries: clz(c), 33 = empty tile."""
    c = int(c)
    return 32 - c.bit_length() if c else LPT_BUCKETS - 1


def chunk_rows(T):
    """make_dims: depth-ordered Gaussians per count-table row."""
    return (4 if T > 1024 else 1) * SLOTS


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
    chunk = chunk_rows(T)
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


def batch_image_layout(W, H, B):
    """carve_image of make_dims(B, ., W, H): every per-pixel and per-tile slab holds B frames back to
    back; strip_hist is per frame 8 queues x 129 buckets (queue map 2: list offsets after
    k_strip_qscan), strip_list_bwd the backward's own tile-major list."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return _carve([("final_T", np.float32, B * W * H), ("n_contrib", np.uint32, B * W * H),
                   ("ranges", np.uint32, 2 * B * T), ("tile_count", np.uint32, B * T),
                   ("work_list", np.uint32, B * T), ("lpt_hist", np.uint32, B * LPT_BUCKETS),
                   ("strip_cnt", np.uint32, 4 * B * T), ("strip_list", np.uint32, 4 * B * T),
                   ("strip_hist", np.uint32, B * 8 * STRIP_BUCKETS), ("strip_list_bwd", np.uint32, 4 * B * T)])


def bin_layout(R):
    n = max(R, 1)
    return _carve([("point_list", np.uint32, n)])


def decode_batch_workspace(r, geom=True):
    """The three arenas of a BatchRasterizer's workspace after a forward (carve_workspace in
    csrc/capi.hip: geometry | image | binning) -> (geometry dict or None, image dict, bin dict).  The
    bin arena is read as point_list[:R] with R the batch total of the control words."""
    B, P, W, H = r.B, r.P, r.W, r.H
    gl, il = geom_layout(P, W, H, B), batch_image_layout(W, H, B)
    gsz, isz = layout_bytes(gl), layout_bytes(il)
    ws = r.workspace
    n4 = 4 * max(r.R_capacity, 1)
    bsz = _align(_align(n4) + n4 if B == 1 else n4) + 256  # carve_bin: a quad-mask slab after the list at B = 1
    assert gsz + isz + bsz + 256 == ws.numel(), ("the layouts are out of step with carve_workspace",
                                                 gsz, isz, bsz, ws.numel())
    R = int(np.frombuffer(ws[:4].cpu().numpy().tobytes(), np.uint32)[CTRL_R])
    assert R <= r.R_capacity, (R, r.R_capacity)
    gs = decode(ws[:gsz].cpu().numpy(), gl) if geom else None
    im = decode(ws[gsz:gsz + isz].cpu().numpy(), il)
    bn = decode(ws[gsz + isz:gsz + isz + 4 * max(R, 1)].cpu().numpy(), bin_layout(R))
    bn["point_list"] = bn["point_list"][:R]
    bn["R"] = R
    return gs, im, bn


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


# ------------------------------------------------------------------ wide-angle and close cameras
#
# camera.camera has tanfovx == tanfovy == 1/24 at distance 22: on every scene above |t.x / t.z| stays
# below 0.73 (x) / 0.955 (y) of the EWA limit 1.3 tanfov, no Gaussian is nearer than z = 21, and the
# perspective column of the projection's Jacobian carries next to nothing.  The two scenes below
# leave that regime; tests/test_oracle.py pins the oracle on them against float64 autograd and
# tests/test_gpu_wide_camera.py the GPU.

def fov_camera(W, H, tanfovx, tanfovy, yaw=0.0, pitch=0.0, distance=22.0):
    """camera.camera with a field of view per axis: the view of camera.look_at_w2c, the projection
    get_proj_matrix(1.0) with P[0,0] = 1 / tanfovx and P[1,1] = 1 / tanfovy."""
    from guava_renderer_amd import camera
    w2c = camera.look_at_w2c(yaw, pitch, distance)
    view = camera.get_view_matrix(w2c[:3, :3], w2c[:3, 3]).T.copy()
    proj = camera.get_proj_matrix(1.0)
    proj[0, 0] = np.float32(1.0) / np.float32(tanfovx)
    proj[1, 1] = np.float32(1.0) / np.float32(tanfovy)
    full = (view @ proj.T.copy()).astype(np.float32)
    c2w = np.linalg.inv(w2c.astype(np.float64)).astype(np.float32)
    return dict(image_height=int(H), image_width=int(W), tanfovx=float(np.float32(tanfovx)),
                tanfovy=float(np.float32(tanfovy)), viewmatrix=view, projmatrix=full, campos=c2w[:3, 3].copy())


def world_z_for_view_z(d, m, zv):
    """World z that puts points (x, y from m) at view-space depth zv (row-vector view matrix,
    graphics_utils.py:44-50 layout: z_view = x V[0][2] + y V[1][2] + z V[2][2] + V[3][2])."""
    V = d["viewmatrix"].astype(np.float64).reshape(4, 4)
    z = (zv - m[:, 0] * V[0, 2] - m[:, 1] * V[1, 2] - V[3, 2]) / V[2, 2]
    return z.astype(np.float32)


def view_space(d):
    """float64 view-space positions [P,3] of the scene's means."""
    V = d["viewmatrix"].astype(np.float64).reshape(4, 4)
    return d["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]


def _bg_and_cotangents(W, H, seed=3):
    rng = np.random.default_rng(seed)
    bg = rng.uniform(-1.0, 2.0, C).astype(np.float32)
    dL = rng.normal(size=(C, H, W)).astype(np.float32)
    dLinv = rng.normal(size=(1, H, W)).astype(np.float32)
    return bg, dL, dLinv


WIDE_TANFOV = (0.8, 0.5)
WIDE_CAMERA = dict(distance=1.6, yaw=0.3, pitch=-0.2)


def wide_cloud(P=400, seed=5):
    """scenes.random_cloud spread over x in +-2.0, y in -0.6 +- 1.3, z in +-0.5 (beyond both EWA limits
    of a camera at distance 1.6 with tanfov (0.8, 0.5)), the first 15% of the Gaussians large (scales
    0.125..0.25: footprints of a hundred pixels), and quaternions of norm 0.6..1.6 (the reference does
    not normalise them)."""
    from guava_renderer_amd import scenes
    d = scenes.random_cloud(P, seed)
    rng = np.random.default_rng(seed + 1)
    m = d["means3D"]
    m[:, 0] = rng.uniform(-2.0, 2.0, P)
    m[:, 1] = rng.uniform(-1.3, 1.3, P) - 0.6
    m[:, 2] = rng.uniform(-0.5, 0.5, P)
    n_big = (3 * P) // 20
    d["scales"][:n_big] = (rng.uniform(0.5, 1.0, (n_big, 3)) * 0.25).astype(np.float32)
    d["rotations"] = (d["rotations"] * rng.uniform(0.6, 1.6, (P, 1))).astype(np.float32)
    return d


def wide_scene(P=400, W=64, H=48, seed=5):
    """Scene "wide": wide_cloud under fov_camera(tanfov (0.8, 0.5), distance 1.6, yaw 0.3, pitch -0.2)
    -> (scene dict with a non-zero bg, dL[C,H,W], dLinv[1,H,W])."""
    d = wide_cloud(P, seed)
    d.update(fov_camera(W, H, *WIDE_TANFOV, **WIDE_CAMERA))
    d["bg"], dL, dLinv = _bg_and_cotangents(W, H)
    return d, dL, dLinv


NEAR_PLANE = np.float32(0.2)   # in_frustum culls view z <= 0.2f (auxiliary.h:151-176)
NEAR_LADDER = 20               # rows of near_scene placed around the near plane
NEAR_CLOSE = 60                # rows behind them placed on screen at view z 0.205..0.4


def near_scene(P=500, W=50, H=38, seed=8):
    """Scene "near": a cloud of small Gaussians around a camera half a unit from its centre (tanfov
    0.6), so that a quarter of them lie behind the near plane.
    The first NEAR_LADDER rows sit near the optical axis at view depths around 0.2f, nextafter(0.2f)
    on both sides, and 0.21: for each of the four depths, the five consecutive float32 world z
    around the solution of world_z_for_view_z (the view transform rounds, so a single solve need not
    land on the depth it aims at; the ladder's steps are smaller than 3 ulp of 0.2f in view z).
    The next NEAR_CLOSE rows are on screen at view z 0.205..0.4.
    The features are halved and the seed chosen so that the oracle's f32 image error against float64
    (rounding of the means amplified by focal / z; 0.8e-5..1.9e-5 over seeds 6..17 even so) stays a
    factor two inside test_oracle._torch_check's 2e-5: 9.8e-6 at this seed.
    -> (scene dict with a non-zero bg, dL, dLinv)."""
    from guava_renderer_amd import scenes
    d = scenes.random_cloud(P, seed)
    rng = np.random.default_rng(seed + 1)
    m = d["means3D"]
    m[:, 0] = rng.uniform(-0.5, 0.5, P)
    m[:, 1] = rng.uniform(-0.4, 0.4, P) - 0.6
    m[:, 2] = rng.uniform(-0.6, 0.6, P)
    d["scales"] = (d["scales"] * np.float32(0.15)).astype(np.float32)
    d.update(fov_camera(W, H, 0.6, 0.6, yaw=-0.2, pitch=0.1, distance=0.5))
    n = NEAR_LADDER
    targets = np.repeat(np.array([NEAR_PLANE, np.nextafter(NEAR_PLANE, np.float32(-1)),
                                  np.nextafter(NEAR_PLANE, np.float32(1)), np.float32(0.21)], np.float64), n // 4)
    V = d["viewmatrix"].astype(np.float64).reshape(4, 4)
    tv = np.stack([rng.uniform(-0.05, 0.05, n), rng.uniform(-0.04, 0.04, n), targets], 1)
    m[:n] = ((tv - V[3, :3]) @ np.linalg.inv(V[:3, :3])).astype(np.float32)
    z = world_z_for_view_z(d, m[:n], targets)
    for _ in range(2):
        z = np.nextafter(z, np.float32(-np.inf))
    for k in range(n):
        for _ in range(k % 5):
            z[k] = np.nextafter(z[k], np.float32(np.inf))
    m[:n, 2] = z
    # on screen just behind the plane: where 1 / t.z^2 and 1 / t.z^3 of the backward are largest
    k = NEAR_CLOSE
    zc = rng.uniform(0.205, 0.4, k)
    tc = np.stack([rng.uniform(-0.5, 0.5, k) * zc, rng.uniform(-0.5, 0.5, k) * zc, zc], 1)
    m[n:n + k] = ((tc - V[3, :3]) @ np.linalg.inv(V[:3, :3])).astype(np.float32)
    d["colors"] = (d["colors"] * np.float32(0.5)).astype(np.float32)
    d["bg"], dL, dLinv = _bg_and_cotangents(W, H)
    return d, dL, dLinv


def wide_conditions(d, radii, g_means3D):
    """What scene "wide" must provide, from the oracle's radii and the float64 means3D gradient alone
    (asserted): -> the counts, for the record."""
    t = view_space(d)
    ax, ay = np.abs(t[:, 0] / t[:, 2]), np.abs(t[:, 1] / t[:, 2])
    lx, ly = 1.3 * d["tanfovx"], 1.3 * d["tanfovy"]
    vis = np.asarray(radii) > 0
    cx, cy = ax > lx, ay > ly
    big = np.abs(g_means3D).max(1) >= 1e-2 * np.abs(g_means3D).max()
    n = dict(visible=int(vis.sum()), clamped=int((vis & (cx | cy)).sum()),
             clamped_with_gradient=int((vis & (cx | cy) & big).sum()),
             clamped_one_axis=int((vis & (cx ^ cy)).sum()),
             swap_changes_decision=int((vis & ((cx != (ax > ly)) | (cy != (ay > lx)))).sum()))
    print("  wide scene: " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert n["clamped_with_gradient"] >= 10 and n["clamped_one_axis"] >= 10 and n["swap_changes_decision"] >= 10, n
    return n


def near_conditions(d, radii):
    """What scene "near" must provide, from the oracle's radii alone (asserted): at least 50 Gaussians
    culled by the near plane, at least 50 visible ones nearer than z = 0.4, and among the ladder rows
    both culled and visible ones with the nearest visible within 4 ulp of 0.2f."""
    z = view_space(d)[:, 2]
    vis = np.asarray(radii) > 0
    assert not vis[z <= 0.2 - 1e-6].any()
    lad = np.arange(len(z)) < NEAR_LADDER
    n = dict(visible=int(vis.sum()), culled_by_near_plane=int((z <= 0.2 - 1e-6).sum()),
             visible_below_0p4=int((vis & (z < 0.4)).sum()), ladder_visible=int((vis & lad).sum()),
             ladder_culled=int((~vis & lad).sum()), nearest_visible=float(z[vis].min()))
    print("  near scene: " + ", ".join(f"{k} {v}" for k, v in n.items()))
    assert n["culled_by_near_plane"] >= 50 and n["visible_below_0p4"] >= 50, n
    assert n["ladder_visible"] >= 5 and n["ladder_culled"] >= 5, n
    assert n["nearest_visible"] <= float(NEAR_PLANE) + 4 * float(np.spacing(NEAR_PLANE)), n
    return n


F64_NAMES = ("colors", "opacity", "means3D", "scales", "rotations", "means2D")


def float64_reference(d, st, dL=None, dLinv=None, scale_modifier=1.0, antialiasing=False, **switches):
    """tests/torch_ref.py on the scene, over the tile lists of the oracle state `st`: (image
    [C,H,W], n_contrib [H*W], gradients by F64_NAMES or None without dL), numpy float64.  "scales" is
    the gradient w.r.t. scale_modifier * scales and "means2D" the NDC one, as the reference returns
    them (torch_ref's docstring).  switches: torch_ref.project's clamp= and diagonal_J=."""
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
                           antialiasing=antialiasing, **switches)
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
