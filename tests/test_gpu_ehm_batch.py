"""The batched EHM deformation (gsr_ehm_forward at more than 16 frames: coefficient tiles, paired
blend, joints regressed in the chains' launches -- csrc/deform.hip ehm_batch_run) against itself
under batch splits and frame permutations (bitwise), against the CPU oracle (2e-5 absolute, as
tests/test_gpu_deform.py), and on a NaN-filled workspace (every word the blends read is written on
every call: the body pose width 486 and the FLAME pose width 36 leave k tails, 17 and 33 frames
leave partial frame tiles).  Synthetic avatar.ehm_assets (SMPL-X / FLAME sizes, 350 coefficients).
"""
import numpy as np
import pytest
import torch

import lbs_oracle as lo

pytestmark = pytest.mark.gpu
ATOL = 2e-5
DEV = "cuda:0"
KEYS = ("vertices", "joints", "joints_transform", "ver_transform_mat", "joint_transform_mat")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def rig():
    """The deformer, 40 frames of parameters and the oracle's outputs of the first 33 (frames are
    independent, so a prefix of the parameters gives a prefix of the outputs)."""
    from guava_renderer_amd import avatar, deform
    body, flame, extra = avatar.ehm_assets(seed=0)
    ehm = deform.EHMDeformer(body, flame, extra["smplx2flame_ind"], extra["l_eyelid"], extra["r_eyelid"], device=DEV)
    bp, fp = avatar.ehm_params(40, seed=6100)
    ref = lo.ehm_forward(body, flame, extra, {k: v[:33] for k, v in bp.items()}, {k: v[:33] for k, v in fp.items()})
    return ehm, bp, fp, ref


def _run(ehm, bp, fp, rows, one_row=(), absent=(), fn="forward"):
    """Frames `rows` (a slice or an index array) in one call; `one_row` parameters keep only their
    first row (broadcast over the frames), `absent` ones are left out."""
    def pick(d):
        return {k: _t(v[:1] if k in one_row else v[rows]) for k, v in d.items() if k not in absent}
    out = getattr(ehm, fn)(pick(bp), pick(fp))
    return {k: out[k].cpu().numpy() for k in KEYS}


@pytest.mark.parametrize("variant", ["per_frame", "broadcast_rows"])
def test_batch_composition_bitwise(rig, variant):
    """40 frames in one call equal frames [0, 20) and [20, 40) in two calls: both sizes take the
    matrix-core blends, whose k split is chosen per model and not per batch, and a frame's MFMA row
    does not depend on its neighbours.  Also with a one-row head_scale and joints_offset and no
    global_pose."""
    ehm, bp, fp, _ = rig
    kw = dict(one_row=("head_scale", "joints_offset"), absent=("global_pose",)) if variant == "broadcast_rows" else {}
    whole = _run(ehm, bp, fp, slice(0, 40), **kw)
    lo_half, hi_half = _run(ehm, bp, fp, slice(0, 20), **kw), _run(ehm, bp, fp, slice(20, 40), **kw)
    for k in KEYS:
        np.testing.assert_array_equal(whole[k][:20], lo_half[k], err_msg=k)
        np.testing.assert_array_equal(whole[k][20:], hi_half[k], err_msg=k)


def test_frame_permutation_bitwise(rig):
    """33 frames (a full 32-frame tile and a one-frame tile): permuting the input rows permutes the
    outputs."""
    ehm, bp, fp, _ = rig
    perm = np.roll(np.arange(33)[::-1], 5)  # (the one-frame tile gets frame 5, frame 32 lands in the full tile)
    base = _run(ehm, bp, fp, np.arange(33))
    got = _run(ehm, bp, fp, perm)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], base[k][perm], err_msg=k)


@pytest.mark.parametrize("B", [17, 33])
def test_matches_oracle(rig, B):
    """17 frames (the smallest matrix-core batch, one partial tile) and 33, against the oracle."""
    ehm, bp, fp, ref = rig
    got = _run(ehm, bp, fp, slice(0, B))
    for k in KEYS:
        err = np.abs(got[k] - ref[k][:B]).max()
        print(f"B={B} {k}: max abs err {err:.3e}")
        np.testing.assert_allclose(got[k], ref[k][:B], atol=ATOL, rtol=0, err_msg=k)
    assert int(ehm.bad.item()) == 0


@pytest.mark.parametrize("B", [17, 33])
def test_poisoned_workspace(rig, B):
    """The cached workspace filled with NaN between two calls: the second call's outputs are finite
    and equal to the first's, so no blend reads a padding or k-tail word that no producer wrote."""
    ehm, bp, fp, _ = rig
    first = _run(ehm, bp, fp, slice(0, B))
    poisoned = 0
    for key, ws in ehm._ws.items():
        if key[0] == B:
            ws.view(torch.float32).fill_(float("nan"))
            poisoned += 1
    assert poisoned >= 1
    again = _run(ehm, bp, fp, slice(0, B))
    for k in KEYS:
        assert np.isfinite(again[k]).all(), k
        np.testing.assert_array_equal(again[k], first[k], err_msg=k)


def test_one_call_equals_per_step_calls_b17(rig):
    """gsr_ehm_forward's fused order against the same steps as separate gsr_lbs_sp /
    gsr_blend_joints_sp / gsr_splice_head calls with caller-owned row-major betas (the launch before
    each blend re-lays them as tiles): bit-identical."""
    ehm, bp, fp, _ = rig
    one = _run(ehm, bp, fp, slice(0, 17))
    steps = _run(ehm, bp, fp, slice(0, 17), fn="forward_calls")
    for k in KEYS:
        np.testing.assert_array_equal(one[k], steps[k], err_msg=k)


@pytest.fixture(scope="module")
def lbs_case():
    from guava_renderer_amd import avatar
    verts, _, _ = avatar.template_mesh()
    m = avatar.lbs_model(verts, J=55, NB=350, seed=0)
    betas = np.random.default_rng(11).normal(size=(17, 350)).astype(np.float32)
    pose = avatar.random_pose(17, seed=1700)
    return m, betas, pose


def _lbs_sp(m, betas, pose, pose2rot, v_template):
    """gsr_lbs_sp with the model's sparse assets and tiled bases (what EHMDeformer prepares per
    model): with more than 16 frames this is the coefficient-tile path -- k_lbs_coef_tiles re-lays
    the caller's row-major betas and forms the pose features from `pose`, k_lbs_blend_tiledc blends,
    and the chain takes its rotations from `pose` and regresses the joints itself.
    Returns (verts, J_transformed, J, T, A) as numpy."""
    import ctypes
    from guava_renderer_amd import _lib, deform
    L = _lib.load()
    B = pose.shape[0]
    Jn, V = m["J_regressor"].shape
    sp, keep = deform.sparse_lbs_assets(m["J_regressor"], m["lbs_weights"], torch.device(DEV))
    assert sp.skin_k > 0
    sd_t = deform._shapedirs_t(_t(m["shapedirs"]))
    pd = _t(m["posedirs"]).float().contiguous()
    tl = [deform.tile_base(sd_t), deform.tile_base(pd)]
    sp.shapedirs_tiled, sp.posedirs_tiled = tl[0].data_ptr(), tl[1].data_ptr()
    (sp.shapedirs_tiled_k, sp.shapedirs_tiled_m), (sp.posedirs_tiled_k, sp.posedirs_tiled_m) = (
        tuple(sd_t.shape), tuple(pd.shape))
    NB = betas.shape[1] if betas is not None else 0
    bt = _t(betas) if betas is not None else None
    vt = _t(v_template)
    gp, jreg, wt = _t(pose), _t(m["J_regressor"]), deform._weights_t(_t(m["lbs_weights"]))
    par = np.ascontiguousarray(m["parents"], np.int32)
    o = dict(dtype=torch.float32, device=DEV)
    verts, jt, jr = torch.empty((B, V, 3), **o), torch.empty((B, Jn, 3), **o), torch.empty((B, Jn, 3), **o)
    T, A = torch.empty((B, V, 4, 4), **o), torch.empty((B, Jn, 4, 4), **o)
    ws = torch.empty((L.gsr_lbs_workspace_bytes(B, V, Jn, NB),), dtype=torch.uint8, device=DEV)
    ws.view(torch.float32).fill_(float("nan"))  # (a fresh allocation may hold anything: make it the worst)
    p = deform._ptr
    rc = L.gsr_lbs_sp(B, V, Jn, NB, p(vt), 0 if vt.dim() == 2 else V * 3, p(bt), p(sd_t) if betas is not None else None,
                      p(gp), 1 if pose2rot else 0, p(pd), p(jreg), par.ctypes.data_as(ctypes.c_void_p), p(wt), None,
                      p(verts), p(jt), p(jr), p(T), p(A), None, p(ws), ctypes.byref(sp), deform._stream(torch.device(DEV)))
    _lib.check(rc, "gsr_lbs_sp")
    torch.cuda.synchronize()
    del keep, tl
    return [x.cpu().numpy() for x in (verts, jt, jr, T, A)]


def test_lbs_sp_tiled_with_row_major_betas_b17(lbs_case):
    """gsr_lbs_sp on tiled bases with caller-owned row-major betas at 17 frames (the relayout in
    k_lbs_coef_tiles, the tiled blend of 350 + 486 coefficients, joints in the chain) against the
    oracle."""
    m, betas, pose = lbs_case
    got = _lbs_sp(m, betas, pose, True, m["v_template"])
    r_verts, r_jt, r_J, r_T, r_A, _ = lo.lbs(betas, pose, m["v_template"], m["shapedirs"], m["posedirs"],
                                             m["J_regressor"], m["parents"], m["lbs_weights"])
    for g, r, name in zip(got, (r_verts, r_jt, r_J, r_T, r_A), ("verts", "J_transformed", "J", "T", "A")):
        assert np.isfinite(g).all(), name
        np.testing.assert_allclose(g, r, atol=ATOL, rtol=0, err_msg=name)


def test_lbs_sp_tiled_rotmat_poses_b17(lbs_case):
    """The same entry with rotation-matrix poses (pose2rot = 0) and no betas (lbs_wobeta): the pose
    features of k_lbs_coef_tiles and the chain's rotations both come straight from the matrices."""
    m, _, pose = lbs_case
    rot = lo.batch_rodrigues(pose.reshape(-1, 3)).reshape(17, 55, 3, 3).astype(np.float32)
    vs = (np.broadcast_to(m["v_template"], (17,) + m["v_template"].shape)
          + np.random.default_rng(3).normal(0, 1e-3, (17,) + m["v_template"].shape)).astype(np.float32)
    got = _lbs_sp(m, None, rot, False, vs)
    ref = lo.lbs_wobeta(rot, vs, m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], pose2rot=False)
    for g, r, name in zip(got, ref, ("verts", "J_transformed", "J", "T", "A")):
        assert np.isfinite(g).all(), name
        np.testing.assert_allclose(g, r, atol=ATOL, rtol=0, err_msg=name)


def test_public_lbs_with_betas_b17(lbs_case):
    """deform.lbs with caller-owned row-major betas at 17 frames, against the oracle (gsr_lbs without
    tiled bases: the k-major matrix-core blend, whose launches this file's other tests do not run)."""
    from guava_renderer_amd import deform
    m, betas, pose = lbs_case
    verts, jt = deform.lbs(_t(betas), _t(pose), _t(m["v_template"]), _t(m["shapedirs"]), _t(m["posedirs"]),
                           _t(m["J_regressor"]), torch.from_numpy(m["parents"]), _t(m["lbs_weights"]))
    r_verts, r_jt, *_ = lo.lbs(betas, pose, m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"],
                               m["parents"], m["lbs_weights"])
    np.testing.assert_allclose(verts.cpu().numpy(), r_verts, atol=ATOL, rtol=0)
    np.testing.assert_allclose(jt.cpu().numpy(), r_jt, atol=ATOL, rtol=0)


def test_public_lbs_wobeta_rotmat_b17(lbs_case):
    """deform.lbs_wobeta with rotation-matrix poses (pose2rot = 0) at 17 frames, against the oracle
    (the k-major path, as above)."""
    from guava_renderer_amd import deform
    m, _, pose = lbs_case
    rot = lo.batch_rodrigues(pose.reshape(-1, 3)).reshape(17, 55, 3, 3).astype(np.float32)
    vs = np.broadcast_to(m["v_template"], (17,) + m["v_template"].shape).astype(np.float32)
    out = deform.lbs_wobeta(_t(rot), _t(vs), _t(m["posedirs"]), _t(m["J_regressor"]), torch.from_numpy(m["parents"]),
                            _t(m["lbs_weights"]), pose2rot=False)
    ref = lo.lbs_wobeta(rot, vs, m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"], pose2rot=False)
    for g, r, name in zip(out, ref, ("verts", "J_transformed", "J", "T", "A")):
        np.testing.assert_allclose(g.cpu().numpy(), r, atol=ATOL, rtol=0, err_msg=name)
