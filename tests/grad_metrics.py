"""Test helper: error metrics for gradient tensors [B, G, ...] (bodies x joints / components / columns).

`relerr` is the tensor-max error every older test here defines for itself: max |got - ref| / max |ref|.  It hides the small joints: the
float64 oracle's |d rotmats| runs from 72 at the root to 0.7 at joint 15 on the inputs of test_smpl_backward_vs_oracle_autograd, so a
block of joint 15 may be 1 % wrong and pass a 1e-4 bar on the tensor maximum.

`slice_errors` adds, with NO element left out,
  - 'group': for each index g of dimension 1 (joint, shape component, column), max over bodies and the group's entries of |got - ref|,
             divided by the maximum of |ref| over the same entries;
  - 'body' : the same with the roles of dimensions 0 and 1 exchanged.
Dense mode (sparse=False): every scale is the slice's own maximum, no floor; a zero scale is an error of the INPUT (the CPU tests of the
case matrices assert that no scale is below 1e-3 of its tensor's maximum).
Sparse mode (one-hot / single-tile upstream gradients, where most of the result is structurally zero and the rest spans four decades):
where the reference's scale is exactly zero the values must be exactly zero (reported as 'nonzero_where_zero'); every other scale is
max(own maximum, 1e-3 x tensor maximum) -- a clamp, not an exclusion: such cases exist to catch a wrong index, which changes whole
values, not last bits.
"""
import numpy as np
import torch

SPARSE_CLAMP = 1e-3


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _np64(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def slice_scales(ref):
    """-> (tensor max, per-group maxima [G], per-body maxima [B]) of |ref|, ref [B, G, ...]"""
    r = np.abs(_np64(ref))
    r = r.reshape(r.shape[0], r.shape[1], -1)
    return float(r.max()) if r.size else 0.0, r.max(axis=(0, 2)), r.max(axis=(1, 2))


def slice_errors(got, ref, sparse=False):
    """-> {'tensor': float, 'group': [G], 'body': [B], 'nonzero_where_zero': int}"""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    g, r = g.reshape(g.shape[0], g.shape[1], -1), r.reshape(r.shape[0], r.shape[1], -1)
    d = np.abs(g - r)
    d[np.isnan(d)] = np.inf                                        # a NaN (an element never written) is an infinite error
    tmax, sg, sb = slice_scales(r)
    eg, eb = d.max(axis=(0, 2)), d.max(axis=(1, 2))
    bad = 0
    if sparse:
        zg, zb = sg == 0, sb == 0
        bad = int((g[:, zg] != 0).sum() + (g[zb] != 0).sum())       # compared by value: -0.0 passes
        sg, sb = np.maximum(sg, SPARSE_CLAMP * tmax), np.maximum(sb, SPARSE_CLAMP * tmax)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = {'tensor': float(d.max() / tmax) if tmax > 0 else (0.0 if d.max() == 0 else np.inf),
               'group': np.where(sg > 0, eg / sg, np.where(eg == 0, 0.0, np.inf)),
               'body': np.where(sb > 0, eb / sb, np.where(eb == 0, 0.0, np.inf)), 'nonzero_where_zero': bad}
    return out


def worst(e):
    return max(float(e['tensor']), float(np.max(e['group'])), float(np.max(e['body'])))


def assert_slices(name, got, ref, ceiling, sparse=False, ref32=None, multiple=None, floor=0.0, ratios=None):
    """every tensor / group / body error of `got` against `ref` (float64) is at most `ceiling`, and -- given the float32 evaluation
    `ref32` of the same reference -- at most multiple x (ref32's error of that slice) + floor.  Prints the figures before it asserts;
    `ratios` (a list) receives (name, kind, index, err, err32) of the slice with the largest (err - floor) / err32."""
    e = slice_errors(got, ref, sparse)
    print('%-44s tensor %.2e  worst group %.2e (#%d)  worst body %.2e (#%d)' % (name, e['tensor'], e['group'].max(), int(e['group'].argmax()),
                                                                               e['body'].max(), int(e['body'].argmax())))
    assert e['nonzero_where_zero'] == 0, '%s: %d values are not zero where the reference is structurally zero' % (name, e['nonzero_where_zero'])
    e32 = slice_errors(ref32, ref, sparse) if ref32 is not None else None
    for kind in ('tensor', 'group', 'body'):
        err = np.atleast_1d(np.asarray(e[kind], np.float64))
        i = int(err.argmax())
        assert err[i] <= ceiling, '%s: %s %d: error %.3e exceeds %.1e' % (name, kind, i, err[i], ceiling)
        if e32 is None:
            continue
        err32 = np.atleast_1d(np.asarray(e32[kind], np.float64))
        over = np.maximum(err - floor, 0.0)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(over > 0, over / err32, 0.0)
        k = int(ratio.argmax())
        if ratios is not None:
            ratios.append((float(ratio[k]), name, kind, k, float(err[k]), float(err32[k])))
        if multiple is not None:
            allowed = multiple * err32 + floor
            w = int((err - allowed).argmax())
            assert err[w] <= allowed[w], ('%s: %s %d: error %.3e exceeds %d x the float32 oracle\'s %.3e + %.1e'
                                          % (name, kind, w, err[w], multiple, err32[w], floor))
    return e
