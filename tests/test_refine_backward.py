"""CPU tests of the refine-backward C ABI (include/gsr.h gsr_refine_backward_*): the header, the
loader's export list and argtypes agree, the ctypes struct has the C compiler's layout, and every
argument check fails on the host with its message before anything is launched (the pointers here
are small integers that are never dereferenced)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsr_refine_backward_scratch_bytes", "gsr_refine_backward_image", "gsr_refine_backward_rows")


def _declaration(name):
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    m = re.search(r"^[a-z_0-9]+\s+" + name + r"\s*\(([^;]*)\);", hdr, re.M)
    assert m, f"{name} is not declared in include/gsr.h"
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_header_exports_and_argtypes_agree():
    from guava_renderer_amd import _lib
    L = _lib.load()
    for name in NEW:
        params = _declaration(name)
        assert name in _lib.EXPORTS
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), (name, params)
        for decl, ct in zip(params, fn.argtypes):
            if "*" in decl:
                want_ptr = True
            else:
                want_ptr = False
            is_ptr = ct is ctypes.c_void_p or hasattr(ct, "contents")
            assert is_ptr == want_ptr, (name, decl, ct)
            if decl.startswith("int64_t"):
                assert ct is ctypes.c_int64, (name, decl)
            elif decl.startswith("int "):
                assert ct is ctypes.c_int, (name, decl)
    assert L.gsr_refine_backward_scratch_bytes.restype is ctypes.c_size_t
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "Forward-only (inference" not in hdr  # the refine path is documented as differentiable


def test_desc_struct_matches_the_c_layout(tmp_path):
    from guava_renderer_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    py, cname = _lib.RefineBackwardDesc, "gsr_refine_backward_desc"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "gsr.h"', "int main(void) {",
             f'printf("size %zu\\n", sizeof({cname}));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l.strip()}
    assert got["size"] == ctypes.sizeof(py)
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f


def _desc(**kw):
    from guava_renderer_amd import _lib
    v = dict(weight=16, n_out=16, keep_channels=4, negative_slope=0.2, pad_=0, out_refine=32, dL_dout_refine=48,
             dL_dkeep=None, dL_dprepared=64, scratch=80)
    v.update(kw)
    return _lib.RefineBackwardDesc(*[v[f] for f, _ in _lib.RefineBackwardDesc._fields_])


IMAGE_CASES = [
    (dict(weight=None), b"null weight or scratch"),
    (dict(scratch=None), b"null weight or scratch"),
    (dict(n_out=0), b"n_out must be >= 1"),
    (dict(n_out=29), b"keep_channels + n_out must be <= 32"),
    (dict(keep_channels=-1), b"keep_channels + n_out must be <= 32"),
    (dict(negative_slope=-0.1), b"negative_slope must be >= 0"),
    (dict(negative_slope=float("nan")), b"negative_slope must be >= 0"),
    (dict(out_refine=None), b"null out_refine"),
    (dict(dL_dout_refine=None), b"null out_refine"),
    (dict(dL_dprepared=None), b"null out_refine"),
]


@pytest.mark.parametrize("change,msg", IMAGE_CASES)
def test_image_end_validates_before_touching_memory(change, msg):
    from guava_renderer_amd import _lib
    L = _lib.load()
    d = _desc(**change)
    rc = L.gsr_refine_backward_image(2, 100, 50, 37, 4096, 1000, ctypes.byref(d), None)
    assert rc == -1 and msg in L.gsr_last_error(), L.gsr_last_error()


def test_image_end_rejects_null_desc_workspace_and_sizes():
    from guava_renderer_amd import _lib
    L = _lib.load()
    d = _desc()
    assert L.gsr_refine_backward_image(2, 100, 50, 37, 4096, 1000, None, None) == -1
    assert b"null desc" in L.gsr_last_error()
    assert L.gsr_refine_backward_image(2, 100, 50, 37, None, 1000, ctypes.byref(d), None) == -1
    assert b"bad batch arguments" in L.gsr_last_error()
    assert L.gsr_refine_backward_image(0, 100, 50, 37, 4096, 1000, ctypes.byref(d), None) == -1
    assert b"bad batch arguments" in L.gsr_last_error()
    assert L.gsr_refine_backward_image(2, 100, 4096, 4096, 4096, 1000, ctypes.byref(d), None) == -1
    assert b"image too large" in L.gsr_last_error()


ROWS_OK = dict(n=64, row_frames=1, d_prepared=256, raw_rows=512, raw_stride=0, B=2, frame_sums=768,
               raw_backgrounds=1024, bg_stride=32, dL_drows=1280, dL_dweight=1536, dL_dbias=None)
ROWS_CASES = [
    (dict(), dict(n_out=0), b"n_out must be >= 1"),
    (dict(), dict(n_out=20, keep_channels=13), b"keep_channels + n_out must be <= 32"),
    (dict(), dict(negative_slope=-1.0), b"negative_slope must be >= 0"),
    (dict(), dict(weight=None), b"null weight or scratch"),
    (dict(d_prepared=None), dict(), b"null d_prepared, raw_rows or dL_drows"),
    (dict(raw_rows=None), dict(), b"null d_prepared, raw_rows or dL_drows"),
    (dict(dL_drows=None), dict(), b"null d_prepared, raw_rows or dL_drows"),
    (dict(dL_dweight=None), dict(), b"null frame_sums, raw_backgrounds or dL_dweight"),
    (dict(frame_sums=None), dict(), b"null frame_sums, raw_backgrounds or dL_dweight"),
    (dict(raw_backgrounds=None), dict(), b"null frame_sums, raw_backgrounds or dL_dweight"),
    (dict(d_prepared=260), dict(), b"16-byte aligned"),
    (dict(raw_rows=520), dict(), b"16-byte aligned"),
    (dict(dL_drows=1284), dict(), b"16-byte aligned"),
    (dict(n=64, row_frames=2, raw_stride=1026), dict(), b"16-byte aligned"),
    (dict(n=65, row_frames=2), dict(), b"row_frames frames"),
    (dict(row_frames=0), dict(), b"row_frames frames"),
    (dict(B=0), dict(), b"row_frames frames"),
]


@pytest.mark.parametrize("args,change,msg", ROWS_CASES)
def test_row_end_validates_before_touching_memory(args, change, msg):
    from guava_renderer_amd import _lib
    L = _lib.load()
    a = dict(ROWS_OK, **args)
    d = _desc(**change)
    rc = L.gsr_refine_backward_rows(a["n"], a["row_frames"], a["d_prepared"], a["raw_rows"], a["raw_stride"], a["B"],
                                    a["frame_sums"], a["raw_backgrounds"], a["bg_stride"], ctypes.byref(d),
                                    a["dL_drows"], a["dL_dweight"], a["dL_dbias"], None)
    assert rc == -1 and msg in L.gsr_last_error(), L.gsr_last_error()
    assert L.gsr_refine_backward_rows(a["n"], a["row_frames"], a["d_prepared"], a["raw_rows"], a["raw_stride"], a["B"],
                                      a["frame_sums"], a["raw_backgrounds"], a["bg_stride"], None, a["dL_drows"],
                                      a["dL_dweight"], a["dL_dbias"], None) == -1
    assert b"null desc" in L.gsr_last_error()


def test_scratch_size_covers_both_ends_and_depends_on_sizes_only():
    """Frame sums [B][64], then the larger of the image end's partial rows (one per 1024 pixels and
    frame) and the row end's partial tiles (one 32x32 tile per workgroup of at least 256 rows)."""
    from guava_renderer_amd import _lib
    L = _lib.load()
    q = L.gsr_refine_backward_scratch_bytes
    assert q(0, 64, 64, 10, 1) == 0 and q(2, 64, 64, 10, 0) == 0
    img = 6 * ((512 * 512 + 1023) // 1024) * 64 * 4
    assert q(6, 512, 512, 1, 1) >= 6 * 64 * 4 + img
    tiles = ((100000 + 255) // 256) * 32 * 32 * 4
    assert q(1, 16, 16, 100000, 1) >= 64 * 4 + tiles
    assert q(6, 512, 512, 600000, 6) >= q(6, 512, 512, 100000, 1)
    assert q(3, 96, 80, 6000, 1) == q(3, 96, 80, 6000, 1)
