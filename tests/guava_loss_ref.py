"""Torch restatement of GUAVA's loss terms beyond the whole-frame L1 (include/gsr_loss.h): the
foreground mask, the head / hand crop losses and the UV-Gaussian regularisers.  Differentiable, any
dtype (the GPU tests run it in float64 on the CPU as the reference of gsr_guava_loss_* and
gsr_uv_regularizers).  The bilinear rule is written out index by index, so the kernels are compared
against the stated rule; test_guava_loss_ref.py checks the rule itself against F.interpolate."""
import torch


def masked_target(target, mask, bg):
    """t = target * mask + (1 - mask) * bg (mask None: the target itself)."""
    return target if mask is None else target * mask + (1.0 - mask) * bg


def axis_taps(n, S, dtype=torch.float64):
    """One axis of upsample_bilinear2d(align_corners=False), input extent n, output S:
    (i0, i1, l0, l1), each [S]."""
    d = torch.arange(S, dtype=dtype)
    scale = torch.tensor(n, dtype=dtype) / S
    src = (scale * (d + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long()
    i1 = i0 + (i0 < n - 1).long()
    l1 = src - i0.to(dtype)
    return i0, i1, 1.0 - l1, l1


def resample(x, S):
    """x [..., h, w] -> [..., S, S] by the rule of axis_taps on both axes."""
    h, w = x.shape[-2:]
    y0, y1, ly0, ly1 = axis_taps(h, S, x.dtype)
    x0, x1, lx0, lx1 = axis_taps(w, S, x.dtype)

    def row(r):
        return lx0 * r[..., x0] + lx1 * r[..., x1]
    return ly0[:, None] * row(x[..., y0, :]) + ly1[:, None] * row(x[..., y1, :])


def clamp_box(box, H, W):
    """(left, right, top, bottom) clamped to the image, or None for a box that is skipped."""
    l, r, t, b = (int(v) for v in box)
    l, r = min(max(l, 0), W), min(max(r, 0), W)
    t, b = min(max(t, 0), H), min(max(b, 0), H)
    return (l, r, t, b) if r > l and b > t else None


def crops(image, boxes, S):
    """image [B,3,H,W], boxes [B,4] -> list (length B) of the resampled cuts [3,S,S], None where skipped."""
    H, W = image.shape[-2:]
    out = []
    for b in range(image.shape[0]):
        bx = clamp_box(boxes[b], H, W)
        out.append(None if bx is None else resample(image[b, :, bx[2]:bx[3], bx[0]:bx[1]], S))
    return out


def crop_l1(image, t, boxes, S, diffs=None):
    """sum|crop(image) - crop(t)| / (n_valid * 3 * S^2) of one group and one image (0 when every box is skipped)."""
    ci, ct = crops(image, boxes, S), crops(t, boxes, S)
    d = [a - b for a, b in zip(ci, ct) if a is not None]
    if not d:
        return image.sum() * 0.0
    d = torch.stack(d)
    if diffs is not None:
        diffs.append(d.detach())
    return d.abs().sum() / (d.shape[0] * 3 * S * S)


def image_loss(feat, target, refine_w, l1_weight, refine_weight, mask=None, bg=0.0, mask_refined=False,
               boxes=None, group_weight=None, S=16, diffs=None):
    """The frame and crop terms of include/gsr_loss.h.  feat [B,32,H,W], target [B,3,H,W], refine_w
    [3,32] or None, mask [B,1,H,W] or None, boxes [G,B,4] (integers) or None, group_weight [G].
    diffs: a list that receives every difference an absolute value is taken of."""
    t = masked_target(target, mask, bg)
    images = [(feat[:, :3], l1_weight)]
    if refine_w is not None:
        r = torch.einsum("oc,bchw->bohw", refine_w, feat)
        if mask is not None and mask_refined:
            r = r * mask + (1.0 - mask) * bg
        images.append((r, refine_weight))
    loss = 0.0
    for im, w in images:
        d = im - t
        if diffs is not None:
            diffs.append(d.detach())
        loss = loss + w * d.abs().mean()
        if boxes is not None:
            for g in range(len(boxes)):
                loss = loss + w * float(group_weight[g]) * crop_l1(im, t, boxes[g], S, diffs)
    return loss


def regularizers(local_pos, uv_scales, xyz_threshold, xyz_weight, scale_threshold, scale_weight):
    """(xyz term, scale term) of the UV-Gaussian regularisers."""
    a = torch.relu(local_pos.norm(dim=-1) - xyz_threshold).mean() * xyz_weight
    b = torch.relu(uv_scales - scale_threshold).norm(dim=-1).mean() * scale_weight
    return a, b
