"""CPU: the stem data-gradient entry points (straps_stem_dgrad*, ABI 12) -- exports, bindings and argument validation are host code,
checkable without a GPU (every check runs before the first HIP call, so the pointers below are never dereferenced)."""
import re

import pytest

from straps_amd import hipabi

EINVAL = 1
NAMES = ['straps_stem_dgrad_weight_floats', 'straps_pack_stem_dgrad_weight', 'straps_stem_dgrad']


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _err(lib):
    return lib.straps_last_error().decode()


def test_symbols_exported_and_bound(lib):
    header = open(hipabi.HEADER).read()
    for n in NAMES:
        assert n in hipabi.SIGNATURES, n
        assert getattr(lib, n) is not None
        assert re.search(r'\b%s\(' % n, header), n
    assert int(re.search(r'#define STRAPS_STEM_DGRAD_MAX_CIN (\d+)', header).group(1)) == 64
    assert lib.straps_abi_version() == hipabi.ABI_VERSION == 12


def test_weight_floats(lib):
    # [64 K groups][ceil(cin / 20) channel chunks][5 tiles][64 lanes][4]
    assert lib.straps_stem_dgrad_weight_floats(18) == 64 * 1 * 5 * 256
    assert lib.straps_stem_dgrad_weight_floats(1) == 64 * 1 * 5 * 256
    assert lib.straps_stem_dgrad_weight_floats(21) == 64 * 2 * 5 * 256
    assert lib.straps_stem_dgrad_weight_floats(64) == 64 * 4 * 5 * 256
    for bad in (0, -1, 65):
        assert lib.straps_stem_dgrad_weight_floats(bad) == 0


P = 4096      # a non-null dummy pointer


@pytest.mark.parametrize('args,msg', [
    ((None, P, P, 2, 18, 256, 256, 0), 'null pointer'),
    ((P, None, P, 2, 18, 256, 256, 0), 'null pointer'),
    ((P, P, None, 2, 18, 256, 256, 0), 'null pointer'),
    ((P, P, P, 0, 18, 256, 256, 0), 'bad shape'),
    ((P, P, P, -3, 18, 256, 256, 0), 'bad shape'),
    ((P, P, P, 2, 0, 256, 256, 0), 'bad shape'),
    ((P, P, P, 2, -1, 256, 256, 0), 'bad shape'),
    ((P, P, P, 2, 65, 256, 256, 0), 'above the supported 64'),
    ((P, P, P, 2, 18, 6, 256, 0), 'bad shape'),
    ((P, P, P, 2, 18, 256, 6, 0), 'bad shape'),
    ((P, P, P, 2, 18, 0, 0, 0), 'bad shape'),
    ((P, P, P, 2, 18, 256, 256, 2), 'accumulate'),
])
def test_stem_dgrad_argument_checks(lib, args, msg):
    assert lib.straps_stem_dgrad(*args, None) == EINVAL
    e = _err(lib)
    assert e.startswith('straps_stem_dgrad:') and msg in e, e


@pytest.mark.parametrize('args,msg', [
    ((None, P, 18), 'null pointer'),
    ((P, None, 18), 'null pointer'),
    ((P, P, 0), 'outside 1..64'),
    ((P, P, 65), 'outside 1..64'),
])
def test_pack_argument_checks(lib, args, msg):
    assert lib.straps_pack_stem_dgrad_weight(*args, None) == EINVAL
    e = _err(lib)
    assert e.startswith('straps_pack_stem_dgrad_weight:') and msg in e, e
