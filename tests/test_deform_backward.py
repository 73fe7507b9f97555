"""CPU tests of the differentiable Gaussian assembly: the float64 reference of its gradient tests
(tests/deform_ref.py) is the oracle's forward and has a correct autograd; the two new entry points
(gsr_deform_gaussians_backward, gsr_backward_batch_deformed) validate on the host before any
launch; the ctypes mirror of GsrDeformGrads has the C layout."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import deform_cases
import deform_ref
import lbs_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _consts(c):
    return deform_ref.Constants(c["verts"], c["vert_transforms"], c["faces"], c["binding_face"], c["face_bary"])


@pytest.mark.parametrize("per_frame", [(), deform_cases.ATTRS])
def test_reference_forward_is_the_oracle(per_frame):
    c = deform_cases.make_case(1, 50, 40, 90, 3, per_frame=per_frame)
    out = deform_ref.forward(_consts(c), *[torch.tensor(c[k], dtype=torch.float64) for k in deform_cases.ATTRS])
    ref = lo.deform_gaussians(c["verts"], c["vert_transforms"], c["faces"], c["vtx_rotations"], c["vtx_scales"],
                              c["binding_face"], c["face_bary"], c["local_xyz"], c["uv_rotations"], c["uv_scales"])
    for got, key in zip(out, ("xyz", "rotation", "scaling")):
        assert np.abs(got.numpy() - ref[key]).max() <= 1e-12, key


def test_reference_autograd_passes_gradcheck():
    c = deform_cases.make_case(2, 12, 8, 20, 2)
    k = _consts(c)
    leaves = [torch.tensor(c[a], dtype=torch.float64, requires_grad=True) for a in deform_cases.ATTRS]
    assert torch.autograd.gradcheck(lambda *a: deform_ref.forward(k, *a), leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("seed,V,F,N,B,sort", [(3, 400, 600, 1500, 3, False), (4, 400, 600, 1500, 9, False),
                                               (5, 300, 500, 1100, 9, True), (6, 70, 40, 300, 1, False)])
def test_gpu_case_inputs_keep_their_decision_margins(seed, V, F, N, B, sort):
    """A condition on the GPU tests' inputs: rotation gradients are compared where the quaternion
    decision margin is >= 1e-4 in every frame, and that must be more than 99% of the Gaussians; the
    unsorted cases' blocks bind face runs > 256 (per-Gaussian face frames), the sorted one's <= 256."""
    c = deform_cases.make_case(seed, V, F, N, B, sort_bindings=sort)
    firm = (_consts(c).margin >= 1e-4).all(0)
    print(f"seed {seed}: {100 * firm.mean():.2f}% kept; face runs {min(deform_cases.block_face_runs(c))}-"
          f"{max(deform_cases.block_face_runs(c))}")
    assert firm.mean() > 0.99
    runs = deform_cases.block_face_runs(c)
    if sort:
        assert max(runs) <= 256
    elif N >= 1500:
        assert min(runs) > 256


def test_new_entry_points_validate_before_touching_memory():
    """Null dg, negative sizes, a stride that is neither 0 nor a whole frame, and a non-zero stride
    passed to the fused call are GSR_ERR_ARG on the host (the pointers here are never dereferenced)."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    bogus = 256
    V, F, N, B = 4, 2, 3, 2

    def inputs(**kw):
        di = _lib.DeformInputs(V, F, N, 0, bogus, bogus, bogus, bogus, 0, bogus, 0, bogus, bogus, bogus, 0, bogus,
                               0, bogus, 0, None)
        for k, v in kw.items():
            setattr(di, k, v)
        return di

    dgr = _lib.DeformGrads(bogus, bogus, bogus, bogus, bogus)

    def bwd(di, B=B, grads=dgr):
        return L.gsr_deform_gaussians_backward(B, ctypes.byref(di) if di is not None else None, bogus, bogus, bogus,
                                               ctypes.byref(grads) if grads is not None else None, None)

    def fused(di, cs=0, os_=0, grads=dgr):
        return L.gsr_backward_batch_deformed(B, 16, 16, ctypes.byref(di) if di is not None else None, bogus, bogus,
                                             bogus, bogus, cs, bogus, os_, 1.0, bogus, bogus, bogus, bogus, 0, bogus,
                                             1024, bogus, None, bogus, bogus,
                                             ctypes.byref(grads) if grads is not None else None, 0, 0, None)

    for call in (bwd, fused):
        assert call(None) == -1 and b"null deform inputs" in L.gsr_last_error()
        assert call(inputs(V=-1)) == -1 and b"bad sizes" in L.gsr_last_error()
        assert call(inputs(N=-2)) == -1 and b"bad sizes" in L.gsr_last_error()
        assert call(inputs(faces=None)) == -1 and b"UV Gaussians" in L.gsr_last_error()
        assert call(inputs(vert_transforms=None)) == -1 and b"vertex Gaussians" in L.gsr_last_error()
        for name, full in (("vtx_rot_stride", 4 * V), ("vtx_scale_stride", 3 * V), ("local_stride", 3 * N),
                           ("uv_rot_stride", 4 * N), ("uv_scale_stride", 3 * N)):
            assert call(inputs(**{name: full + 1})) == -1 and b"whole frame" in L.gsr_last_error(), name
        assert call(inputs(), grads=None) == -1 and b"null gradient" in L.gsr_last_error()
    assert bwd(inputs(), B=0) == -1 and b"bad sizes" in L.gsr_last_error()
    # the fused call takes shared attributes only: any whole-frame stride is refused there
    for name, full in (("vtx_rot_stride", 4 * V), ("vtx_scale_stride", 3 * V), ("local_stride", 3 * N),
                       ("uv_rot_stride", 4 * N), ("uv_scale_stride", 3 * N)):
        assert fused(inputs(**{name: full})) == -1 and b"shared by every frame" in L.gsr_last_error(), name
    assert fused(inputs(), cs=32 * (V + N)) == -1 and b"shared by every frame" in L.gsr_last_error()
    assert fused(inputs(), os_=V + N) == -1 and b"shared by every frame" in L.gsr_last_error()
    assert fused(inputs(), grads=_lib.DeformGrads(bogus, None, bogus, bogus, bogus)) == -1 and \
        b"null canonical gradient" in L.gsr_last_error()


def test_deform_grads_struct_matches_the_c_layout(tmp_path):
    from guava_renderer_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    py = _lib.DeformGrads
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gsr_deform.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(GsrDeformGrads));']
    lines += [f'printf("{f} %zu\\n", offsetof(GsrDeformGrads, {f}));' for f, _ in py._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["size"] == ctypes.sizeof(py)
    assert [f for f, _ in py._fields_] == ["vtx_rotations", "vtx_scales", "local_xyz", "uv_rotations", "uv_scales"]
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f


def test_autograd_surface_refuses_a_mesh_gradient():
    """deform_gaussians raises before any GPU work when verts / vert_transforms require grad."""
    from guava_renderer_amd import deform
    z = torch.zeros
    args = [z(1, 4, 3), z(1, 4, 4, 4), z(2, 3, dtype=torch.int32), z(3, dtype=torch.int32), z(3, 3), z(4, 4),
            z(4, 3), z(3, 3), z(3, 4), z(3, 3)]
    args[0].requires_grad_(True)
    with pytest.raises(NotImplementedError):
        deform.deform_gaussians(*args)
    args[0] = z(1, 4, 3)
    args[1].requires_grad_(True)
    with pytest.raises(NotImplementedError):
        deform.deform_gaussians(*args)
