"""Seeded inputs shared by the UV Gaussian extraction's CPU and GPU tests (test_gaussian_extract_ref.py,
test_gpu_gaussian_extract.py).  Everything is numpy; arrays handed out by the cached builders are
read-only.

Maps: raw head outputs of plausible spread (opacity logits N(0, 3), log-scales N(-4, 1), quaternions
N(0, 1), colours N(0, 1.5), local positions N(0, 0.01)), planar [B,k,U,U]; the rows-activated form of
the same case is the restatement's activations of them, laid out [B,U,U,k], as the decoder returns.
"""
import functools

import numpy as np

import gaussian_extract_ref as ref

KEYS = ref.KEYS
MASKS = ("full", "empty", "last", "random", "stripes")
STRIPE_RUNS = (1, 63, 64, 65, 63, 1, 65, 64)  # on, off, on, ...: on-runs 1, 64, 63, 65 straddle tile borders


def mask(kind, T, seed=0):
    """uint8 [T]."""
    m = np.zeros(T, np.uint8)
    if kind == "full":
        m[:] = 1
    elif kind == "last":
        m[T - 1] = 1
    elif kind == "first":
        m[0] = 1
    elif kind == "random":
        n = 769 if T == 1024 else (3 * T) // 4 + 1
        m[np.random.default_rng(seed).choice(T, n, replace=False)] = 1
    elif kind == "stripes":
        t, i = 0, 0
        while t < T:
            run = STRIPE_RUNS[i % len(STRIPE_RUNS)]
            if i % 2 == 0:
                m[t:t + run] = 1
            t += run
            i += 1
    else:
        assert kind == "empty", kind
    return m


def widths(C):
    return dict(colors=C, opacities=1, scales=3, rotations=4, local_pos=3)


def raw_maps(B, U, C, seed):
    """dict of planar raw maps [B,k,U,U] float32."""
    rng = np.random.default_rng(seed)
    spread = dict(colors=(0.0, 1.5), opacities=(0.0, 3.0), scales=(-4.0, 1.0), rotations=(0.0, 1.0), local_pos=(0.0, 0.01))
    return {k: (spread[k][0] + spread[k][1] * rng.standard_normal((B, w, U, U))).astype(np.float32)
            for k, w in widths(C).items()}


def activated_rows(raw):
    """The decoder's outputs [B,U,U,k] of raw planar maps: the restatement's activations, no RGB sigmoid."""
    B, _, U, _ = raw["colors"].shape
    act = ref.activate(ref.to_rows(raw, True), True, False)
    return {k: np.ascontiguousarray(v).reshape(B, U, U, -1) for k, v in act.items()}


def special_maps(U, C):
    """B = 1 raw maps whose first texels carry NaN, +-inf, +-200, +-0 and subnormal logits and zero,
    subnormal and huge quaternions; the rest is the seeded case."""
    m = {k: v.copy() for k, v in raw_maps(1, U, C, seed=77).items()}
    vals = np.array([np.nan, np.inf, -np.inf, 200.0, -200.0, 0.0, -0.0, 1e-45, -1e-45, 88.8, -88.0, -103.5, -104.5],
                    np.float32)
    n = vals.size
    m["opacities"].reshape(-1)[:n] = vals
    m["scales"].reshape(3, -1)[:, :n] = vals
    m["colors"].reshape(C, -1)[:3, :n] = vals
    m["colors"].reshape(C, -1)[3, :n] = vals  # copied channels keep the bits
    q = m["rotations"].reshape(4, -1)
    q[:, 0] = 0.0
    q[:, 1] = (1e-45, 0.0, 0.0, 0.0)
    q[:, 2] = (1e19, -1e19, 1e19, 1e19)   # the sum of squares overflows
    q[:, 3] = (3e-13, 0.0, 0.0, 0.0)      # below the clamp
    q[:, 4] = (np.nan, 1.0, 0.0, 0.0)
    q[:, 5] = (np.inf, 1.0, 0.0, 0.0)
    return m


def gradients(B, N, C, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((B, N, w)).astype(np.float32) for k, w in widths(C).items()}


def binding(T, seed):
    """(texel_face int32 [T], texel_bary float32 [T,3])."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 20908, T).astype(np.int32), rng.dirichlet((1.0, 1.0, 1.0), T).astype(np.float32)


def prune_thresholds(opacity, m):
    """opacity float32 [T] (the restatement's activated opacities), m uint8 [T] -> dict name -> (threshold,
    kept count) with kept counts 0, 1, N and about N/2.  Asserts, on the restatement alone, that no
    masked opacity lies within 3 * 2^-23 relative of a threshold, so that the strict comparison has
    one answer under the stated error of the sigmoid."""
    o = np.sort(opacity[m != 0].astype(np.float64))
    N = o.size
    assert N >= 4 and o[0] > 0 and np.all(np.diff(o[[0, 1, N // 2 - 1, N // 2, N - 2, N - 1]]) > 0)
    mid = lambda a, b: np.float32(0.5 * (a + b))  # noqa: E731
    out = dict(none=(np.float32(min(1.0, o[-1] * 1.001)), 0), one=(mid(o[-2], o[-1]), 1),
               all=(np.float32(o[0] * 0.5), N), half=(mid(o[N // 2 - 1], o[N // 2]), N - N // 2))
    for name, (thr, kept) in out.items():
        assert np.abs(o - float(thr)).min() > 3 * 2.0 ** -23 * float(thr), name
        assert int((opacity[m != 0] > thr).sum()) == kept, name
    return out


@functools.lru_cache(maxsize=None)
def case(U, B, C, kind, seed=5):
    """One seeded case, made once: dict of mask [T], raw (planar maps), rows (activated maps),
    texel_face, texel_bary, N."""
    T = U * U
    raw = raw_maps(B, U, C, seed + U + 7 * B + C)
    rows = activated_rows(raw)
    m = mask(kind, T, seed)
    tf, tb = binding(T, seed + 1)
    for a in list(raw.values()) + list(rows.values()) + [m, tf, tb]:
        a.setflags(write=False)
    return dict(mask=m, raw=raw, rows=rows, texel_face=tf, texel_bary=tb, N=int(m.sum()), U=U, B=B, C=C)
