"""CPU checks of tests/guava_loss_ref.py, the torch restatement that the GPU tests of the GUAVA loss
kernels compare against: its bilinear rule is F.interpolate(mode='bilinear') (the reference's
cal_box_loss resampling), and empty boxes are skipped as include/gsr_loss.h states."""
import pytest
import torch
import torch.nn.functional as F

import guava_loss_ref as ref


@pytest.mark.parametrize("h,w,S", [(9, 7, 16), (40, 37, 16), (1, 5, 16), (5, 1, 16), (32, 32, 32), (48, 64, 16),
                                   (150, 61, 256)])
def test_resample_is_interpolate_bilinear(h, w, S):
    x = torch.rand((3, h, w), dtype=torch.float64, generator=torch.Generator().manual_seed(h * 100 + w))
    want = F.interpolate(x[None], (S, S), mode="bilinear")[0]
    got = ref.resample(x, S)
    assert got.shape == (3, S, S)
    assert (got - want).abs().max().item() <= 1e-12
    # float32 too (the kernels' format): powers of two S make scale * (d + 0.5) exact
    got32 = ref.resample(x.float(), S)
    want32 = F.interpolate(x.float()[None], (S, S), mode="bilinear")[0]
    assert (got32 - want32).abs().max().item() <= 1e-6


def test_identity_resample():
    x = torch.rand((3, 32, 32), dtype=torch.float64)
    assert torch.equal(ref.resample(x, 32), x)


def test_taps_clamp_at_the_last_index():
    i0, i1, l0, l1 = ref.axis_taps(1, 16)
    assert i0.tolist() == [0] * 16 and i1.tolist() == [0] * 16  # (l1 > 0 for d >= 8: both taps are pixel 0)
    i0, i1, l0, l1 = ref.axis_taps(7, 16)
    assert int(i1.max()) == 6 and int(i0.min()) == 0
    assert torch.allclose(l0 + l1, torch.ones(16, dtype=torch.float64))


def test_boxes_clamp_and_skip():
    assert ref.clamp_box((-5, 70, -2, 100), 48, 64) == (0, 64, 0, 48)
    assert ref.clamp_box((10, 10, 0, 5), 48, 64) is None
    assert ref.clamp_box((10, 5, 0, 5), 48, 64) is None
    assert ref.clamp_box((0, 5, 7, 7), 48, 64) is None
    assert ref.clamp_box((70, 90, 0, 5), 48, 64) is None  # clamps to an empty box


def test_crop_mean_is_over_the_kept_boxes():
    g = torch.Generator().manual_seed(1)
    img = torch.rand((2, 3, 48, 64), dtype=torch.float64, generator=g)
    t = torch.rand((2, 3, 48, 64), dtype=torch.float64, generator=g)
    both = torch.tensor([[3, 20, 5, 30], [10, 40, 2, 20]])
    one = torch.tensor([[3, 20, 5, 30], [10, 10, 2, 20]])
    none = torch.tensor([[3, 3, 5, 30], [10, 40, 20, 20]])
    single = (F.interpolate(img[:1, :, 5:30, 3:20], (16, 16), mode="bilinear") -
              F.interpolate(t[:1, :, 5:30, 3:20], (16, 16), mode="bilinear")).abs().mean()
    assert abs(ref.crop_l1(img, t, one, 16).item() - single.item()) <= 1e-14
    assert ref.crop_l1(img, t, both, 16).item() != ref.crop_l1(img, t, one, 16).item()
    img.requires_grad_(True)
    z = ref.crop_l1(img, t, none, 16)
    z.backward()
    assert z.item() == 0.0 and img.grad.abs().max().item() == 0.0


def test_image_loss_without_mask_and_boxes_is_the_frame_l1():
    g = torch.Generator().manual_seed(2)
    feat = torch.rand((2, 32, 8, 8), dtype=torch.float64, generator=g)
    tgt = torch.rand((2, 3, 8, 8), dtype=torch.float64, generator=g)
    rw = torch.rand((3, 32), dtype=torch.float64, generator=g)
    want = 0.8 * (feat[:, :3] - tgt).abs().mean() + (torch.einsum("oc,bchw->bohw", rw, feat) - tgt).abs().mean()
    assert abs(ref.image_loss(feat, tgt, rw, 0.8, 1.0).item() - want.item()) <= 1e-15
    m = torch.ones((2, 1, 8, 8), dtype=torch.float64)
    assert abs(ref.image_loss(feat, tgt, rw, 0.8, 1.0, mask=m, bg=0.3, mask_refined=True).item() - want.item()) <= 1e-15


def test_regularizers_zero_rows_have_zero_gradient():
    lp = torch.tensor([[0., 0., 0.], [3., 4., 0.], [0.1, 0.1, 0.1]], dtype=torch.float64, requires_grad=True)
    sc = torch.tensor([[0.1, 0.2, 0.3], [0.9, 0.1, 1.0], [0.6, 0.6, 0.6]], dtype=torch.float64, requires_grad=True)
    a, b = ref.regularizers(lp, sc, 3.0, 0.01, 0.6, 1.0)
    (a + b).backward()
    assert abs(a.item() - 0.01 * 2.0 / 3) <= 1e-15 and abs(b.item() - 0.5 / 3) <= 1e-15
    assert torch.isfinite(lp.grad).all() and torch.isfinite(sc.grad).all()
    assert lp.grad[0].abs().max().item() == 0 and sc.grad[0].abs().max().item() == 0 and sc.grad[2].abs().max().item() == 0
