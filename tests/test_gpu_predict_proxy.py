"""GPU: straps_predict_proxy_input (csrc/predict.hip) against the reference's own results (tests/golden/predict_proxy_golden.npz) and the
numpy restatement of the header (tests/predict_cases.py): channel 0 and the heat maps bit for bit, the joints equal to np.float32 of the
reference's float64, the boxes equal; mixed batches and single samples; the two invalid samples beside valid ones; frames whose size is
no multiple of 16 bytes; the real shape.  Every output sits NaN-filled between redzone margins: an element the kernel does not write
shows as NaN, a write outside as a damaged margin."""
import os

import numpy as np
import pytest
import torch

import predict_cases as PC
import straps_amd
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'predict_proxy_golden.npz')
CASES = [(g, o) for g in sorted(PC.GROUPS) for o in PC.GROUPS[g][4]]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    hipabi.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _run(dev, sil, joints, out_wh, std=PC.STD, scale=PC.SCALE):
    """the raw library call on guarded buffers -> numpy (out, joints, boxes)"""
    B, H, W = sil.shape
    nj, ld = joints.shape[1], joints.shape[2]
    z = Zone(dev)
    out = z.guarded((B, 1 + nj, out_wh, out_wh), name='out_nchw')
    jout = z.guarded((B, nj, 2), name='out_joints2d')
    boxes = z.guarded((B, 6), dtype=torch.int32, fill=-77, name='boxes')
    s, j = torch.from_numpy(sil).to(dev), torch.from_numpy(joints).to(dev)
    patch = torch.from_numpy(straps_amd.heatmap_patch(std)).to(dev)
    hipabi.check(hipabi.lib().straps_predict_proxy_input(hipabi.ptr(s), hipabi.ptr(j), ld, hipabi.ptr(patch), std, scale, hipabi.ptr(out),
                                                         hipabi.ptr(jout), hipabi.ptr(boxes), B, H, W, nj, out_wh, hipabi.stream_ptr()),
                 'straps_predict_proxy_input')
    torch.cuda.synchronize()
    z.check()
    return out.cpu().numpy(), jout.cpu().numpy(), boxes.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _assert_equals_restatement(got, sil, joints, out_wh, what, std=PC.STD):
    out, j, boxes = got
    want, wj, wboxes = PC.proxy_input(sil, joints, straps_amd.heatmap_patch(std), out_wh, std=std)
    assert not np.isnan(out).any() and not np.isnan(j).any(), '%s: an output element was not written' % what
    assert np.array_equal(boxes, wboxes), (what, boxes, wboxes)
    assert _same_bits(out[:, 0], want[:, 0]), '%s: channel 0 differs from the restatement' % what
    assert _same_bits(out[:, 1:], want[:, 1:]), '%s: heat maps differ from the restatement' % what
    assert _same_bits(j, wj.astype(np.float32)), '%s: joints differ from the restatement' % what


def _assert_equals_golden(got, gold, group, out_wh, pick, what):
    out, j, boxes = got
    key = '%s_o%d_' % (group, out_wh)
    assert _same_bits(out[:, 0], gold[key + 'sil'][pick].astype(np.float32)), '%s: channel 0 differs from the reference' % what
    assert _same_bits(out[:, 1:], gold[key + 'heat'][pick]), '%s: heat maps differ from the reference' % what
    assert _same_bits(j, gold[key + 'joints'][pick].astype(np.float32)), '%s: joints != np.float32(reference float64)' % what
    assert (boxes[:, 4] == 1).all() and (boxes[:, 5] == 0).all()


@pytest.fixture(scope='module')
def batch_results(dev):
    """the mixed batch of every (group, out_wh), computed once and left unchanged"""
    return {(g, o): _run(dev, *PC.inputs(g), o) for g, o in CASES}


@pytest.mark.parametrize('group,out_wh', CASES)
def test_mixed_batch_against_reference_and_restatement(batch_results, gold, group, out_wh):
    sil, joints = PC.inputs(group)
    got = batch_results[(group, out_wh)]
    _assert_equals_golden(got, gold, group, out_wh, slice(None), 'group %s -> %d' % (group, out_wh))
    _assert_equals_restatement(got, sil, joints, out_wh, 'group %s -> %d' % (group, out_wh))


def test_batch_of_five(batch_results):
    assert batch_results[('a', 32)][0].shape == (5, 18, 32, 32) and batch_results[('a', 64)][0].shape == (5, 18, 64, 64)


@pytest.mark.parametrize('group,out_wh', CASES)
def test_single_samples_against_reference_and_batch(dev, batch_results, gold, group, out_wh):
    """B = 1 for every sample: the reference's result, and bit for bit sample i of the mixed batch"""
    sil, joints = PC.inputs(group)
    whole = batch_results[(group, out_wh)]
    for i, sample in enumerate(PC.GROUPS[group][5]):
        got = _run(dev, sil[i:i + 1], joints[i:i + 1], out_wh)
        _assert_equals_golden(got, gold, group, out_wh, slice(i, i + 1), '%s/%s -> %d alone' % (group, sample[0], out_wh))
        assert _same_bits(got[0], whole[0][i:i + 1]) and _same_bits(got[1], whole[1][i:i + 1]) and np.array_equal(got[2], whole[2][i:i + 1]), sample[0]


@pytest.mark.parametrize('out_wh', [32, 64])
def test_invalid_samples_beside_valid_ones(dev, batch_results, out_wh):
    """an empty silhouette and a one-pixel one (the reference raises on both): all zeros, valid 0; their valid neighbours are unchanged"""
    sil, joints = PC.inputs('a')
    inv = PC.invalid_silhouettes()
    order = [0, 'empty', 1, 'one_pixel', 3]
    s = np.stack([inv[k] if isinstance(k, str) else sil[k] for k in order])
    j = np.stack([joints[2] if isinstance(k, str) else joints[k] for k in order])       # (live joints on the invalid samples: they must come out 0)
    out, jo, boxes = got = _run(dev, s, j, out_wh)
    _assert_equals_restatement(got, s, j, out_wh, 'invalid beside valid -> %d' % out_wh)
    whole = batch_results[('a', out_wh)]
    for pos, k in enumerate(order):
        if isinstance(k, str):
            assert not out[pos].any() and not jo[pos].any() and boxes[pos, 4] == 0 and boxes[pos, 5] == 0, k
            assert np.array_equal(out[pos].view(np.uint32), np.zeros_like(out[pos]).view(np.uint32)), '%s: -0.0 or NaN in a zero output' % k
        else:
            assert _same_bits(out[pos], whole[0][k]) and _same_bits(jo[pos], whole[1][k]) and np.array_equal(boxes[pos], whole[2][k]), k
    assert boxes[1].tolist() == [0, 0, 0, 0, 0, 0] and boxes[3].tolist() == [20, 30, 20, 30, 0, 0]
    # a batch of nothing but invalid samples
    out, jo, boxes = _run(dev, np.stack([inv['empty'], inv['one_pixel']]), j[:2], out_wh)
    assert not out.any() and not jo.any() and not boxes[:, 4].any()


@pytest.mark.parametrize('h,w,nj,ld,out_wh,std', [(37, 53, 2, 2, 32, 4), (5, 3, 1, 3, 4, 4), (33, 47, 3, 2, 20, 4), (64, 64, 17, 3, 32, 3), (40, 40, 2, 2, 48, 1)])
def test_odd_frames_and_other_tables(dev, h, w, nj, ld, out_wh, std):
    """frames of h * w bytes that are no multiple of 16 (samples after the first start unaligned: the byte-wise head and tail of the
    bounding-box sweep), a frame smaller than one 16-byte load, an out_wh that is no multiple of the 16-row tile, other std"""
    rng = np.random.RandomState(h * 100 + w)
    B = 4
    sil = np.zeros((B, h, w), np.uint8)
    for b in range(B):
        r0, c0 = rng.randint(0, h // 2), rng.randint(0, w // 2)
        r1, c1 = rng.randint(r0 + 1, h), rng.randint(c0 + 1, w)
        sil[b] = PC._blob(h, w, r0, r1, c0, c1, b)
    sil[1] = 0
    sil[1, h - 1, w - 1] = sil[1, h - 2, w - 2] = 9              # the last byte of a frame: the tail of the sweep
    sil[2, :, :] = 0
    sil[2, 0, 0] = sil[2, 1, 1] = 3                              # the first byte: the head
    joints = np.stack([PC._scatter_joints(h, w, nj, ld, 50 + b) for b in range(B)])
    _assert_equals_restatement(_run(dev, sil, joints, out_wh, std=std), sil, joints, out_wh, '%dx%d -> %d std %d' % (h, w, out_wh, std), std=std)


def test_real_shape(dev):
    """512 x 512 -> 256, 17 joints with confidence, B = 2: sixteen row tiles per channel; one window inside the frame, one leaving it"""
    sil = np.stack([PC._blob(512, 512, 100, 400, 180, 330, 1), PC._blob(512, 512, 3, 500, 200, 420, 2)])
    joints = np.stack([PC._scatter_joints(512, 512, 17, 3, 7), PC._scatter_joints(512, 512, 17, 3, 8)])
    got = _run(dev, sil, joints, 256)
    _assert_equals_restatement(got, sil, joints, 256, '512 -> 256')
    assert got[2][0, 0] >= 0 and got[2][1, 0] < 0 and got[2][1, 2] > 512
    assert got[0][:, 1:].any(axis=(2, 3)).sum() >= 10            # (most of the scattered joints are drawn)


def test_python_entry_point(dev, batch_results):
    """create_proxy_representation_batch: uint8 / bool / float silhouettes, [B,J,2] and [B,J,3] joints, non-contiguous inputs; the
    patch is cached per (device, std)"""
    sil, joints = PC.inputs('a')
    want = batch_results[('a', 32)]
    s, j = torch.from_numpy(sil).to(dev), torch.from_numpy(joints).to(dev)
    for sv, jv in ((s, j), (s, j[:, :, :2]), (s.float(), j), (s.double(), j.double())):
        out, jo, boxes = straps_amd.create_proxy_representation_batch(sv, jv, out_wh=32)
        assert out.dtype == jo.dtype == torch.float32 and boxes.dtype == torch.int32
        assert _same_bits(out.cpu().numpy(), want[0]) and _same_bits(jo.cpu().numpy(), want[1]) and np.array_equal(boxes.cpu().numpy(), want[2])
    mask = s != 0
    out_b, jo_b, boxes_b = straps_amd.create_proxy_representation_batch(mask, j, out_wh=32)
    out_u, jo_u, boxes_u = straps_amd.create_proxy_representation_batch(mask.to(torch.uint8), j, out_wh=32)
    assert torch.equal(out_b, out_u) and torch.equal(jo_b, jo_u) and torch.equal(boxes_b, boxes_u)
    assert torch.equal(out_b[:, 1:], out[:, 1:]) and set(out_b[:, 0].unique().tolist()) == {0.0, 1.0}
    from straps_amd import predict
    assert predict._device_patch(dev, 4) is predict._device_patch(dev, 4)
    with pytest.raises(RuntimeError):
        straps_amd.create_proxy_representation_batch(s.cpu(), j, out_wh=32)
    with pytest.raises(RuntimeError):
        straps_amd.create_proxy_representation_batch(s, j, out_wh=30)
