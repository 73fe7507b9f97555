"""The scenes of tests/test_gpu_binning_state.py and tests/test_binning_ref.py: scenes.random_cloud
with scaled scales under the canonical camera, per-frame means3D [B, P, 3] whose suffix is moved behind
the camera so that frame b sees exactly V[b] Gaussians (0: an all-empty frame), and optional splats of
a large world-space scale at the cloud's centre (they cover every tile of the grid).  The oracle
state of every frame is computed once per case and shared."""
import functools

import numpy as np

import helpers

C = 32
ATTRS = ("colors", "opacities", "scales", "rotations")
YAWS = (0.0, 0.12, -0.08)


@functools.lru_cache(maxsize=2)  # (a 2048 x 2048 frame of 32 channels is half a gigabyte)
def make_case(W, H, P, seed, scale, V, big=()):
    """V: visible Gaussians wanted per frame (the first V[b] rows of the cloud stay where they are).
    big: world-space scales of rows 0.. (placed at the centre of the cloud).  -> dict with the shared
    attributes, means3D [B, P, 3], the cameras, and per frame the oracle's (colour, radii, inverse
    depth, state) on a zero background."""
    import oracle
    from guava_renderer_amd import camera, scenes
    sc = scenes.random_cloud(P, seed)
    sc["scales"] = (sc["scales"] * np.float32(scale)).astype(np.float32)
    for i, s in enumerate(big):
        sc["scales"][i] = np.float32(s)
        sc["means3D"][i] = (0.0, -0.6, 0.0)
    B = len(V)
    means = np.repeat(sc["means3D"][None], B, 0).copy()
    for b, v in enumerate(V):
        means[b, v:] = (0.0, 0.0, -100.0)  # behind the camera: culled
    cams = [camera.camera(W, H, yaw=YAWS[b % len(YAWS)]) for b in range(B)]
    frames = []
    for b, c in enumerate(cams):
        frames.append(oracle.forward(means[b], sc["colors"], sc["opacities"], sc["scales"], sc["rotations"], None,
                                     c["viewmatrix"], c["projmatrix"], W, H, c["tanfovx"], c["tanfovy"],
                                     np.zeros(C, np.float32)))
    for f in frames:
        for a in f[:3]:
            a.setflags(write=False)
    return dict(W=W, H=H, P=P, B=B, V=tuple(V), sc=sc, means3D=means, cams=cams, frames=frames)


def states(case):
    return [f[3] for f in case["frames"]]


# (id, W, H, P, seed, scale, V per frame, big splats)
ROW1 = [(f"96x80-V{a}-0-{b}", 96, 80, max(a, b) + 40, 50 + i, 1.0, (a, 0, b), ())
        for i, (a, b) in enumerate([(1, 64), (64, 256), (256, 257), (257, 511), (511, 512), (512, 513), (513, 1)])]
ROW2 = [(f"528x512-V{a}-{b}", 528, 512, max(a, b) + 40, 60 + i, 0.5, (a, b), (3.0, 3.0))
        for i, (a, b) in enumerate([(255, 1025), (256, 2600), (257, 2049), (1023, 256), (1024, 1280), (1025, 255),
                                    (1280, 2048), (2048, 1023), (2049, 257), (2600, 1024)])]
ROW3 = [("16x16400", 16, 16400, 2000, 71, 1.0, (2000, 1300), ()),
        ("16400x16", 16400, 16, 2000, 72, 1.0, (2000, 1300), ())]
ROW4 = [("2048x2048", 2048, 2048, 1300, 81, 2.0, (1300,), (3.0,)),
        ("4096x1024", 4096, 1024, 600, 82, 2.0, (600,), (3.0,))]
ROW5 = [(f"528x512-single-V{v}", 528, 512, v + 40, 90 + i, 0.5, (v,), (3.0, 3.0)) for i, v in enumerate((1024, 1025, 2600))]


def regime(case, ref):
    """What the reference says the case reaches: per frame V, count-table rows and the passes of the
    last row, plus the batch's full-grid splats -- the figures of the printed regime line."""
    fr = ref["frames"]
    return dict(V=[f["V"] for f in fr], chunk=ref["chunk"], nchunk=-(-case["P"] // ref["chunk"]),
                rows=[f["nrows"] for f in fr], passes=[f["passes"] for f in fr],
                full_grid=[f["full_grid"] for f in fr], R=[f["R"] for f in fr])


def pass_loop_exit(V):
    """How the last count-table row of a frame of V visible Gaussians leaves k_ordered_scatter's pass
    loop at T > 1024 (1024-Gaussian rows, 256 per pass): its last pass partial or full, and by the
    j0 >= V break (fewer than four passes) or by the loop count."""
    last = V - (V - 1) // 1024 * 1024
    passes = -(-last // 256)
    return ("partial" if last % 256 else "full") + ("+break" if passes < 4 else "+count")
