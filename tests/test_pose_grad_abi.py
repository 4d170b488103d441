"""CPU: the axis-angle gradient entry points (straps_rodrigues_bwd, straps_smpl_bwd_aa) are exported and validate their arguments
before any HIP call (no compute calls -- there is no GPU here)."""
import ctypes as C

import pytest

from straps_amd import hipabi

EINVAL = 1


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def test_symbols_exported_and_bound(lib):
    for n in ('straps_rodrigues_bwd', 'straps_smpl_bwd_aa'):
        assert hasattr(lib, n), 'library does not export %s' % n
        assert n in hipabi.SIGNATURES


def test_rodrigues_bwd_argument_checks(lib):
    f = C.c_void_p(16)           # never dereferenced: validation fails first
    for args in ((None, f, f, 4), (f, None, f, 4), (f, f, None, 4)):
        assert lib.straps_rodrigues_bwd(*args, None) == EINVAL
        assert b'straps_rodrigues_bwd' in lib.straps_last_error() and b'null pointer' in lib.straps_last_error()
    for n in (0, -3):
        assert lib.straps_rodrigues_bwd(f, f, f, n, None) == EINVAL
        assert b'n must be positive' in lib.straps_last_error()


def _bwd_tables(ms):
    for name in ('blend_frag_t', 'children', 'jrt_ptr', 'dj_ptr', 'dj_code', 'dj_w'):
        setattr(ms, name, 16)


def test_smpl_bwd_aa_argument_checks(lib):
    ms = hipabi.SmplModelStruct()
    _bwd_tables(ms)
    f = C.c_void_p(16)
    good = [C.byref(ms), f, f, f, f, f, f, f, None, f, 4, 0, None]
    # model, betas, rotmats, full_pose_aa, dbetas, dfull_pose_aa, workspace are required (dverts / djoints / drotmats may be NULL)
    for i in (1, 2, 3, 6, 7, 9):
        args = list(good)
        args[i] = None
        assert lib.straps_smpl_bwd_aa(*args) == EINVAL, 'argument %d' % i
        assert b'straps_smpl_bwd_aa: null pointer' in lib.straps_last_error()
    assert lib.straps_smpl_bwd_aa(None, *good[1:]) == EINVAL
    for batch in (0, -1):
        args = list(good)
        args[10] = batch
        assert lib.straps_smpl_bwd_aa(*args) == EINVAL
        assert b'batch must be positive' in lib.straps_last_error()
    # a model struct without the backward tables
    bare = hipabi.SmplModelStruct()
    assert lib.straps_smpl_bwd_aa(C.byref(bare), *good[1:]) == EINVAL
    assert b'backward tables' in lib.straps_last_error()


def test_axis_angle_grad_path_refuses_cpu_and_fp64_before_any_launch(monkeypatch):
    """SMPL(pose2rot=True) with grad and batch_rodrigues with grad check their inputs before the first library call: a CPU tensor (a body_pose
    left on the host in fitting code) raises 'GPU tensor' instead of reaching a kernel as a host pointer."""
    import torch
    import straps_amd

    def no_launch():
        raise AssertionError('a library call was reached before the input check')
    monkeypatch.setattr(hipabi, 'lib', no_launch)
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=2)        # (module Parameters on the CPU, requiring grad)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        smpl(betas=torch.zeros(2, 10))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        smpl(betas=torch.zeros(2, 10), body_pose=torch.zeros(1, 69, requires_grad=True), global_orient=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        straps_amd.batch_rodrigues(torch.zeros(4, 3, requires_grad=True))
    with pytest.raises(RuntimeError, match='GPU tensor'):
        from straps_amd.autograd_ops import smpl_aa_forward_autograd
        smpl_aa_forward_autograd(smpl, torch.zeros(2, 10), torch.zeros(2, 72, requires_grad=True))
