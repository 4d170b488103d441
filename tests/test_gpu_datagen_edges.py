"""GPU: straps_crop_resize (csrc/image.hip), straps_augment_seg and the two deviation kernels (csrc/augment.hip) off the 256-pixel frame,
against the oracle with the draws supplied: both sweeps of crop_bbox_kernel (float4 and scalar) with fewer and with more pixels than its
1024 threads, silhouettes that are empty, one pixel, one row, one column, the whole frame or pressed against a border, output sizes from 1
to 37, occlusion boxes of 0, 1, 3 and 0.7 wh pixels in frames of 5 to 100, batches of 1 to 1000.  Every output sits between redzone
margins, pre-filled with a value the kernel never writes; every operand ends directly in front of a poisoned margin."""
import numpy as np
import pytest
import torch

import datagen_cases as DC
import straps_oracle as O
from detgen import det_uniform
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
SCALE, DS, DC_RANGE = 1.2, (-0.2, 0.2), (-5.0, 5.0)      # the training configuration's box scale and jitter ranges


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


def _f32(a):
    return torch.from_numpy(np.array(a, np.float32))


# ---- crop + resize -----------------------------------------------------------------------------------------------------------------
def _crop(dev, seg, joints, u, out_wh):
    """the raw call: seg [B,wh,wh], joints [B,nj,2], u [B,3] or None -> (map, joints, boxes [B,6]) numpy.  out, jout and boxes are guarded;
    seg, joints and the draws end in front of NaN (a NaN read past the last image counts as foreground and moves the box)"""
    B, wh, nj = seg.shape[0], seg.shape[-1], joints.shape[1]
    z = Zone(dev)
    out, jout = z.guarded((B, out_wh, out_wh), name='out'), z.guarded((B, nj, 2), name='jout')
    boxes = z.guarded((B, 6), dtype=torch.int32, fill=-77, name='boxes')
    s, j, ud = z.at_end(_f32(seg)), z.at_end(_f32(joints)), None if u is None else z.at_end(_f32(u))
    hipabi.check(hipabi.lib().straps_crop_resize(hipabi.ptr(s), hipabi.ptr(j), hipabi.ptr(ud), SCALE, DS[0], DS[1], DC_RANGE[0], DC_RANGE[1], hipabi.ptr(out),
                                                 hipabi.ptr(jout), hipabi.ptr(boxes), B, wh, out_wh, nj, hipabi.stream_ptr()), 'straps_crop_resize')
    torch.cuda.synchronize()
    z.check()
    out, jout, boxes = out.cpu().numpy(), jout.cpu().numpy(), boxes.cpu().numpy()
    assert not np.isnan(out).any() and not np.isnan(jout).any() and (boxes != -77).all(), 'an output element was not written'
    return out, jout, boxes


def _crop_batches(wh, B):
    """the crop cases in batches of B images: each case alone, or three neighbours of the table (the last batch wraps round)"""
    cases = DC.crop_cases(wh)
    names = list(DC.CROP_CASES)
    if B == 1:
        return [((n,), cases[n][None]) for n in names]
    return [(tuple(names[(i + k) % len(names)] for k in range(B)), np.stack([cases[names[(i + k) % len(names)]] for k in range(B)]))
            for i in range(0, len(names), B)]


@pytest.mark.parametrize('out_wh', (1, 5, 32, 37))
@pytest.mark.parametrize('wh', (6, 7, 30, 33, 64, 68))
def test_crop_resize_off_the_training_frame(dev, wh, out_wh):
    """boxes [:, :4] and the resized map exact, joints to rtol 1e-5 / atol 1e-3, against O.crop_resize fed the same float32 draws as
    float64.  wh 6 / 7 and 33: the scalar sweep with fewer and with more pixels than the 1024 threads; wh 30: scalar (30 % 4 = 2); wh 64:
    the float4 sweep in exactly one trip; wh 68: with a ragged second trip.
    The reference does NOT pin two kinds of case, which it cannot process; for them the test asserts what the kernel documents: an empty
    frame keeps the whole frame as its box (0, 0, wh, wh) and gives an all-zero map; a crop of zero size (a single pixel) gives an all-zero
    map and joints (j - corner) * out_wh.  Their boxes still follow the reference's arithmetic (DC.crop_expected)."""
    pinned_seen = unpinned_seen = 0
    for nj in (1, 17):
        for B in (1, 3):
            joints = DC.crop_joints(B, nj, wh)
            for u in (None, DC.crop_draws(B)):
                for names, seg in _crop_batches(wh, B):
                    got, gj, gb = _crop(dev, seg, joints, u, out_wh)
                    assert (gb[:, 4:6] == gb[:, 0:2]).all()
                    for i, name in enumerate(names):
                        want, wj, wb, pinned = DC.crop_expected(seg[i], joints[i], None if u is None else u[i], out_wh)
                        what = (name, 'nj %d' % nj, 'B %d' % B, 'jitter' if u is not None else 'no jitter')
                        assert np.array_equal(gb[i, :4], wb), (what, gb[i].tolist(), wb.tolist())
                        assert np.array_equal(got[i], want), (what, int((got[i] != want).sum()))
                        np.testing.assert_allclose(gj[i], wj, rtol=1e-5, atol=1e-3, err_msg=str(what))
                        if name == 'empty':
                            assert gb[i].tolist() == [0, 0, wh, wh, 0, 0] and not got[i].any()
                        pinned_seen += pinned
                        unpinned_seen += not pinned
    assert pinned_seen >= 4 * 8 and unpinned_seen >= 8 * 4          # (8 of the 12 cases are pinned without jitter; 2 x 2 x 2 passes over the table)


# ---- part removal + occlusion box --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wh', (5, 33, 64, 100))
def test_augment_seg_off_the_training_frame(dev, wh):
    """exact against O.augment_seg, B in (1, 3), box_dim in (0, 1, 3, floor(0.7 wh)), on part maps with ids 0..8 (7 and 8 survive removal).
    box_dim stays at or below 0.7 wh: beyond that a corner of the box goes negative, where the reference's numpy slice wraps round and the
    kernel clamps; the training configuration (256, 48) never gets there, and this test does not go there either."""
    L = hipabi.lib()
    probs = _f32(DC.REMOVE_PROBS).to(dev)
    for B in (1, 3):
        for name, (seg, u) in DC.seg_cases(B, wh).items():
            for box in (0, 1, 3, int(np.floor(0.7 * wh))):
                want = O.augment_seg(seg, u, remove_probs=DC.REMOVE_PROBS, occlude_probability=DC.OCCLUDE_PROB, occlude_box_dim=box)
                z = Zone(dev)
                out = z.guarded((B, wh, wh), name='seg out')
                s, ud = z.at_end(_f32(seg)), z.at_end(_f32(u))
                hipabi.check(L.straps_augment_seg(hipabi.ptr(s), hipabi.ptr(ud), hipabi.ptr(probs), DC.OCCLUDE_PROB, box, hipabi.ptr(out), B, wh,
                                                  hipabi.stream_ptr()), 'straps_augment_seg')
                torch.cuda.synchronize()
                z.check()
                got = out.cpu().numpy()
                assert np.array_equal(got, want), (name, B, box, int((got != want).sum()))
                assert ((got == seg) | (got == 0)).all()
                if name == 'all_removed':                             # ids 7 and 8 are no removable class: they survive outside the box
                    assert set(np.unique(got[0]).tolist()) == {0.0, 7.0, 8.0}


# ---- deviation kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 3, 17, 1000))
def test_deviation_kernels_at_small_and_ragged_sizes(dev, n):
    """straps_deviate_joints2d on n bodies and straps_deviate_verts2d on n vertices, exact against the oracle, outputs guarded"""
    L = hipabi.lib()
    j, uj = det_uniform((n, 17, 2), 950 + n, 20.0, 236.0), det_uniform((n, 17, 2), 951 + n, 0.0, 1.0)
    uj[0, 0], uj[0, 11] = (0.0, DC.LAST_DRAW), (DC.LAST_DRAW, 0.0)
    z = Zone(dev)
    out = z.guarded((n, 17, 2), name='joints out')
    jd, ud = z.at_end(_f32(j)), z.at_end(_f32(uj))
    hipabi.check(L.straps_deviate_joints2d(hipabi.ptr(jd), hipabi.ptr(ud), -8.0, 8.0, -15.0, 15.0, hipabi.ptr(out), n, hipabi.stream_ptr()),
                 'straps_deviate_joints2d')
    torch.cuda.synchronize()
    z.check()
    want = O.random_joints2D_deviation(j.copy(), uj.copy(), [-8, 8], [-15, 15]).numpy()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.abs(want - j)[:, [11, 12]].max() <= 15.0 and np.abs(want - j)[:, :11].max() <= 8.0
    v, uv = det_uniform((1, n, 3), 960 + n, -1.0, 1.0), det_uniform((1, n, 2), 961 + n, 0.0, 1.0)
    uv[0, 0] = (0.0, DC.LAST_DRAW)
    z = Zone(dev)
    out = z.guarded((1, n, 3), name='verts out')
    vd, ud = z.at_end(_f32(v)), z.at_end(_f32(uv))
    hipabi.check(L.straps_deviate_verts2d(hipabi.ptr(vd), hipabi.ptr(ud), -0.01, 0.01, hipabi.ptr(out), n, hipabi.stream_ptr()), 'straps_deviate_verts2d')
    torch.cuda.synchronize()
    z.check()
    want = O.random_verts2D_deviation(v.copy(), uv.copy(), (-0.01, 0.01)).numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got[:, :, 2], v[:, :, 2])
