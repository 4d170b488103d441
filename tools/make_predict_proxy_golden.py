"""Writes tests/golden/predict_proxy_golden.npz: what the REFERENCE computes for the cases of tests/predict_cases.py.

    python tools/make_predict_proxy_golden.py --reference /path/to/the/reference/checkout

CPU only.  The reference's own `crop_and_resize_silhouette_joints` (utils/image_utils.py) and `convert_2Djoints_to_gaussian_heatmaps`
(utils/label_conversions.py, called as predict/predict_3D.py:71 calls it: on joints.astype(np.int16)) are imported and run; nothing of
their text is restated here.  OpenCV is not needed: a stand-in `cv2` module provides the two functions and three constants that path
uses -- copyMakeBorder as np.pad, and resize with OpenCV's nearest index rule (src = min(floor(dst * (1 / (dst_size / src_size))),
src_size - 1), as oracle/straps_oracle.py restates it for the training-side crop).

The file holds data only.  Per group g of the case table: g_sil [B,H,W] uint8 and g_joints [B,nj,ld] float32 (the inputs), and per
output size o: g_o<o>_sil [B,o,o] uint8, g_o<o>_joints [B,nj,2] float64, g_o<o>_heat [B,nj,o,o] float32 (the reference's [o,o,nj] maps
with the joint axis moved in front: long runs of zeros compress better)."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def cv2_stand_in():
    m = types.ModuleType('cv2')
    m.BORDER_CONSTANT, m.INTER_NEAREST, m.INTER_LINEAR = 0, 0, 1

    def copyMakeBorder(src, top, bottom, left, right, borderType, value=0):
        assert borderType == m.BORDER_CONSTANT and src.ndim == 2
        return np.pad(src, ((int(top), int(bottom)), (int(left), int(right))), mode='constant', constant_values=value)

    def resize(src, dsize, interpolation=None):
        assert interpolation == m.INTER_NEAREST and src.ndim == 2
        ow, oh = dsize
        sh, sw = src.shape
        if sh <= 0 or sw <= 0:
            raise ValueError('resize: empty source (OpenCV asserts !ssize.empty())')
        ys = np.minimum(np.floor(np.arange(oh) * (1.0 / (oh / float(sh)))).astype(np.int64), sh - 1)
        xs = np.minimum(np.floor(np.arange(ow) * (1.0 / (ow / float(sw)))).astype(np.int64), sw - 1)
        return src[ys][:, xs]

    m.copyMakeBorder, m.resize = copyMakeBorder, resize
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default=os.environ.get('STRAPS_REFERENCE'), help='checkout of the reference project (or $STRAPS_REFERENCE)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'predict_proxy_golden.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(os.path.join(args.reference, 'utils')):
        ap.error('--reference must name a checkout of the reference project')
    sys.modules['cv2'] = cv2_stand_in()
    sys.path.insert(0, args.reference)
    from utils.image_utils import crop_and_resize_silhouette_joints
    from utils.label_conversions import convert_2Djoints_to_gaussian_heatmaps
    import predict_cases as PC

    data = {}
    for g, (H, W, nj, ld, outs, samples) in sorted(PC.GROUPS.items()):
        PC.check_properties(g)
        sil, joints = PC.inputs(g)
        data['%s_sil' % g], data['%s_joints' % g] = sil, joints
        for o in outs:
            rs, rj, rh = [], [], []
            for b in range(sil.shape[0]):
                s, j, _ = crop_and_resize_silhouette_joints(sil[b], joints[b], o, bbox_scale_factor=PC.SCALE)
                heat = convert_2Djoints_to_gaussian_heatmaps(j.astype(np.int16), o)
                assert s.shape == (o, o) and s.dtype == np.uint8 and j.shape == (nj, 2) and j.dtype == np.float64
                assert heat.shape == (o, o, nj) and heat.dtype == np.float32
                rs.append(s)
                rj.append(j)
                rh.append(np.ascontiguousarray(np.transpose(heat, (2, 0, 1))))
            data['%s_o%d_sil' % (g, o)], data['%s_o%d_joints' % (g, o)], data['%s_o%d_heat' % (g, o)] = np.stack(rs), np.stack(rj), np.stack(rh)
    # the two cases the kernel defines as invalid: the reference must raise on them (they are NOT in the file)
    for name, s in PC.invalid_silhouettes().items():
        try:
            crop_and_resize_silhouette_joints(s, np.zeros((17, 2), np.float32), 32)
        except Exception as e:      # noqa: BLE001
            print('reference raises on %s: %s: %s' % (name, type(e).__name__, e))
        else:
            raise SystemExit('the reference completed the %r silhouette: it is not an invalid case' % name)
    np.savez_compressed(args.out, **data)
    print('wrote %s: %d arrays, %d bytes' % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
