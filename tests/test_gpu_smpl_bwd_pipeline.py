"""GPU: the look-ahead of the SMPL gradient kernels (csrc/smpl_bwd.hip) where a ring or a batch of loads can go wrong.

smpl_verts_bwd_kernel keeps RD fragment groups (phase 1) and 4 RD transposed fragments (phase 4) in flight and requests a round's dverts rows,
skinning entries and table ranges ahead of their phases; smpl_pose_bwd_kernel reads the chunk partials PU = 9 chunks at a time, the remainder one
by one (the tests with fewer `chunks` values use 1, PU + 2 and 54: no batch, a batch with a remainder, six batches).  A load past the end of a
table, an input or the workspace reads a NaN margin here (every input ends directly before one, the workspace is exactly straps_smpl_bwd_workspace_bytes long inside redzones: the launch helpers of tests/test_gpu_smpl_bwd_edges.py), and a batch that drops
or repeats a chunk misses the oracle.

  - `chunks` around the batch size of the pose pass -- 1, 2, PU - 1, PU, PU + 1, PU + 2 (one batch and two single chunks), 2 PU (two batches exactly),
    53 and 54 -- at B = 1 and at B = 33 (one full 32-body tile and a tile of one body);
  - dverts NULL with djoints given, and the reverse;
  - a model with 7 skinning weights on some vertices (more than the 4 fetched ahead) and one with a single weight per vertex (fewer);
  - every model's last tile holds 10 vertices (6890 = 215 x 32 + 10).

Reference, metric and bars are those of tests/test_gpu_smpl_bwd_edges.py (CEILING, MULTIPLE, the float32 floor of tests/smpl_cases.py), imported,
not derived again; the oracle gradients are the cached ones of its cases.  Also asserted: three launches give identical bits, straps_smpl_bwd and
straps_smpl_bwd_aa agree bit for bit, and two `chunks` values agree within the bar of that file.
"""
import numpy as np
import pytest
import torch

import grad_metrics as G
import smpl_cases as S
import test_gpu_smpl_bwd_edges as E
from redzone import Zone
from straps_amd import hipabi

pytestmark = pytest.mark.gpu


def _pose_batch():
    """PU of csrc/smpl_bwd.hip, read from the source: the edges below move with it"""
    import os
    import re
    src = open(os.path.join(hipabi.CSRC, 'smpl_bwd.hip')).read()
    return int(re.search(r'constexpr int PU = (\d+);', src).group(1))


PU = _pose_batch()                       # chunk partials per batch of smpl_pose_bwd_kernel
# (a `chunks` request becomes ceil(54 / ceil(54 / chunks)) chunks: PU + 1 = 10 gives 9 again, PU + 2 = 11 gives 11 = one batch and two single chunks)
CHUNKS = (1, 2, PU - 1, PU, PU + 1, PU + 2, 2 * PU, 53, 54)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    hipabi.load()
    before = torch.get_num_threads()
    torch.set_num_threads(S.cpu_threads())
    yield torch.device('cuda:0')
    torch.set_num_threads(before)


def _check(dev, name, kind, chunk_list):
    """case `name` of smpl_cases.CASES with upstream gradient `kind` at every `chunks` of the list"""
    c = S.CASES[name]
    x = S.inputs(name)
    floor = S.float32_floor()
    smpl = E._smpl(dev, c['model'])
    sparse = c['up'] != 'dense'
    d = E._on_device(Zone(dev), x, kind)
    r64, r32 = S.oracle(name, kind, torch.float64), S.oracle(name, kind, torch.float32)
    first = None
    for chunks in chunk_list:
        tag = '%s/%s/chunks=%d' % (name, kind, chunks)
        got = E._launch(smpl, d, chunks, 'aa')
        for _ in range(2):
            assert E._same(E._launch(smpl, d, chunks, 'aa'), got), tag + ': not reproducible'
        rot = E._launch(smpl, d, chunks, 'rot')
        assert torch.equal(rot['dbetas'], got['dbetas']) and torch.equal(rot['drot'], got['drot']), tag + ': the two entry points differ'
        E._against_oracle(tag, got, name, kind, sparse, floor)
        if first is None:
            first = got
            continue
        for k, v in got.items():            # another summation order of the same products: within the measured bar of the first `chunks`
            e, e32 = G.slice_errors(v, first[k], sparse), G.slice_errors(r32[k], r64[k], sparse)
            for part in ('tensor', 'group', 'body'):
                assert np.all(np.asarray(e[part]) <= E.MULTIPLE * np.asarray(e32[part]) + floor), '%s %s: differs from chunks=%d' % (tag, k, chunk_list[0])


@pytest.mark.parametrize('name', ['batch1', 'batch33'])
def test_chunk_counts_around_the_pose_batch(dev, name):
    _check(dev, name, 'both', CHUNKS)


@pytest.mark.parametrize('kind', ['verts', 'joints'])
def test_one_upstream_gradient_absent(dev, kind):
    _check(dev, 'batch33', kind, (1, PU + 2, 54))


@pytest.mark.parametrize('name', ['model_wide', 'model_rigid'])
def test_more_and_fewer_skinning_weights_than_fetched_ahead(dev, name):
    assert E._smpl(dev, S.CASES[name]['model']).skin_k == {'model_wide': 7, 'model_rigid': 1}[name]
    _check(dev, name, 'both', (1, PU + 2, 54))
