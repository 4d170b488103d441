"""Test helper: the case tables of tests/test_gpu_norm_pool_edges.py and a statement of WHICH LOOP FORM of the streaming kernels each case reaches.

The BatchNorm, pooling and pooling-gradient kernels (csrc/elementwise.hip, csrc/backward.hip) are grid-stride loops behind a launch cap; which of
their loop forms runs, for how many trips and with what tail, follows from the launch rules.  This module restates those rules in Python -- limited
to what the tables need:

    straps_grid256, straps_grid256_rows, straps_bn_tiled (product default: mode 1), straps_bn_tiled_grid        csrc/common.h
    capped_grid                                                                                                 csrc/elementwise.hip, csrc/backward.hip
    straps_bn_bwd_blocks, rows_per_block = ceil(rows / nblk), straps_bn_bwd_workspace_bytes                     csrc/backward.hip
    POOL_CHUNK = 1024 (bn_bwd_apply_kernel<true>)                                                               csrc/backward.hip
    the channel rule of straps_bn_bwd (bn_bwd_x3_impl): C4 <= 256 ? 256 % C4 == 0 : C4 % 256 == 0               csrc/backward.hip
    the trip structure of bn_partials_sum4: 64 lane groups, 16 x 64 partial blocks per unrolled trip            csrc/common.h

tests/test_norm_cases_cpu.py holds straps_bn_bwd_blocks and straps_bn_bwd_workspace_bytes to the library for every case.  The tiling and grid rules
(straps_grid256*, straps_bn_tiled*, capped_grid, POOL_CHUNK) are `static inline` / file-local: the library exports nothing that would confirm their
restatement without a launch, and no entry point is added for that -- a change of one of them has to be repeated here by hand; what the GPU tests
then still check is the result, not the form reached.

What a case reaches is named by a tuple:
    (launch site, loop form, trips, tail)
        launch site   'bn_apply'            bn_apply_kernel behind capped_grid (straps_bn_apply)
                      'bn_apply_x3'         bn_apply_kernel behind straps_bn_tiled / straps_grid256_rows (straps_bn_apply_x3, _bits_x3)
                      'bn_bwd_apply'        bn_bwd_apply_kernel<false> (straps_bn_bwd, _x3, _bits_x3, _finish_x3, _finish_bits_x3)
                      'bn_bwd_apply_pool'   bn_bwd_apply_kernel<true>: POOL_CHUNK elements per workgroup, 256 per trip (straps_bn_bwd_pooled[_sparse])
                      'maxpool', 'maxpool_idx', 'bn_relu_maxpool', 'maxpool_bwd', 'gap_bwd'       the per-element loops behind capped_grid
        loop form     'tiled' | 'fixed' (the stride is a multiple of the row: hoisted channel constants, row += rstep) | 'per_element'
        trips         '1' | '>1': whether any thread runs its loop body more than once
        tail          True when the threads of the launch run unequal numbers of trips (the last trip is partial)
    ('bn_bwd_reduce', unrolled, tail, empty)      bn_bwd_reduce_kernel<false>: the four-rows-per-trip loop runs / the tail loop runs / a trailing block
                                                  has r0 >= rows
    ('bn_partials_sum4', unrolled, tail)          the sixteen-loads-per-trip loop runs / the tail loop runs (bn_stats_finalize_kernel, bn_bwd_finalize_kernel)
"""
import itertools
from collections import namedtuple

CAP = 256 * 16                     # workgroups of 256 threads
POOL_CHUNK = 1024
MAX_FLOATS = 20 * 1000 * 1000      # the largest tensor of any case


# ------------------------------------------------------------------------------------------------------------------------------------
# launch rules

def straps_grid256(n):
    """csrc/common.h straps_grid256"""
    g = (n + 255) // 256
    return CAP if g > CAP else (1 if g < 1 else g)


def capped_grid(n):
    """csrc/elementwise.hip and csrc/backward.hip capped_grid: the same rule"""
    return straps_grid256(n)


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def straps_grid256_rows(n, C4):
    """csrc/common.h straps_grid256_rows: grid x 256 a multiple of the row length whenever a grid under the cap allows it"""
    g = straps_grid256(n)
    if C4 > 0 and 256 % C4 != 0:
        m = C4 // _gcd(C4, 256)
        if m <= CAP:
            up = (g + m - 1) // m * m
            g = (CAP // m) * m if up > CAP else up
    return g


def straps_bn_tiled(rows, C4, mode=1):
    """csrc/common.h straps_bn_tiled; mode 1 is the product library's compile-time default"""
    if not mode or (C4 & 15):
        return 0
    ncg = C4 >> 4
    if not (ncg == 1 or ncg == 2 or (ncg & 3) == 0) or (mode == 1 and ncg < 4):
        return 0
    wcg = ncg if ncg < 4 else 4
    return wcg if rows % (16 // wcg) == 0 else 0


def straps_bn_tiled_grid(rows, C4, wcg):
    """csrc/common.h straps_bn_tiled_grid"""
    ncb = (C4 >> 4) // wcg
    tiles = rows // (16 // wcg) * ncb
    g = min(tiles, CAP) // ncb * ncb
    return ncb if g < ncb else g


def straps_bn_bwd_blocks(rows, c):
    """csrc/backward.hip straps_bn_bwd_blocks"""
    colblocks = (c + 63) // 64
    b = min(2048 // colblocks, (rows + 63) // 64)
    return 1 if b < 1 else b


def rows_per_block(rows, c):
    """csrc/backward.hip bn_bwd_x3_impl: rpb"""
    nblk = straps_bn_bwd_blocks(rows, c)
    return (rows + nblk - 1) // nblk


def straps_bn_bwd_workspace_bytes(rows, c):
    """csrc/backward.hip straps_bn_bwd_workspace_bytes: partials [nblk][c][2] and coefficients [2][c] as doubles, k1 [c] as floats"""
    return (straps_bn_bwd_blocks(rows, c) * c * 2 + 2 * c) * 8 + c * 4


def bn_bwd_finish_workspace_bytes(c):
    """csrc/backward.hip straps_bn_bwd_finish_x3: (2 c) doubles + c floats"""
    return 2 * c * 8 + c * 4


def bn_bwd_channels_ok(c):
    """csrc/backward.hip bn_bwd_x3_impl, bn_bwd_finish_x3_impl, straps_bn_bwd_pooled_sparse"""
    C4 = c >> 2
    return c > 0 and c % 4 == 0 and (256 % C4 == 0 if C4 <= 256 else C4 % 256 == 0)


def pool_out(h):
    """3x3 / stride 2 / pad 1"""
    return (h - 1) // 2 + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# what a launch reaches

def _linear(n, grid, C4):
    """a grid-stride loop over n elements, 256 threads per workgroup -> (form, trips, tail)"""
    step = grid * 256
    return ('fixed' if C4 and step % C4 == 0 else 'per_element', '>1' if n > step else '1', n % step != 0)


def _tiled(rows, C4, wcg):
    ncb, trows = (C4 >> 4) // wcg, 16 // wcg
    rstep = straps_bn_tiled_grid(rows, C4, wcg) // ncb * trows
    return ('tiled', '>1' if rows > rstep else '1', rows % rstep != 0)


def bn_apply_reach(entry, rows, c):
    """entry 'plain' (straps_bn_apply) | 'x3' (straps_bn_apply_x3, straps_bn_apply_bits_x3)"""
    C4 = c >> 2
    if entry == 'plain':
        return ('bn_apply',) + _linear(rows * C4, capped_grid(rows * C4), C4)
    wcg = straps_bn_tiled(rows, C4)
    return ('bn_apply_x3',) + (_tiled(rows, C4, wcg) if wcg else _linear(rows * C4, straps_grid256_rows(rows * C4, C4), C4))


def bn_bwd_apply_reach(rows, c):
    C4 = c >> 2
    wcg = straps_bn_tiled(rows, C4)
    return ('bn_bwd_apply',) + (_tiled(rows, C4, wcg) if wcg else _linear(rows * C4, straps_grid256_rows(rows * C4, C4), C4))


def bn_bwd_apply_pool_reach(B, H, W, c):
    """a workgroup owns POOL_CHUNK consecutive float4 elements and walks them 256 at a time: four trips in a whole chunk"""
    C4 = c >> 2
    n4 = B * H * W * C4
    rem = n4 % POOL_CHUNK
    counts = ({POOL_CHUNK // 256} if n4 >= POOL_CHUNK else set()) | ({len(range(t, rem, 256)) for t in (0, 255)} if rem else set())
    return ('bn_bwd_apply_pool', 'fixed' if 256 % C4 == 0 else 'per_element', '>1' if max(counts) > 1 else '1', len(counts) > 1)


def bn_bwd_reduce_reach(rows, c):
    """bn_bwd_reduce_kernel<false>: thread row lane tr = 0..15 of block bx walks r = r0 + tr, r0 + tr + 16, ...; four rows per unrolled trip while
    r + 48 < r1, then one per tail trip"""
    nblk, rpb = straps_bn_bwd_blocks(rows, c), rows_per_block(rows, c)
    lengths, empty = set(), False
    for b in {0, (rows - 1) // rpb, nblk - 1}:                      # a full block (or the only one), the last block with rows, the last block
        r0 = b * rpb
        if r0 >= rows:
            empty = True
        else:
            lengths.add(min(r0 + rpb, rows) - r0)
    unrolled = tail = False
    for L, tr in itertools.product(lengths, range(16)):
        r = tr
        while r + 48 < L:
            unrolled, r = True, r + 64
        tail = tail or r < L
    return ('bn_bwd_reduce', unrolled, tail, empty)


def bn_partials_sum4_reach(nblocks):
    """bn_partials_sum4: lane group pl = 0..63 walks k = pl, pl + 64, ...; sixteen per unrolled trip while k + 960 < nblocks"""
    unrolled = tail = False
    for pl in range(64):
        k = pl
        while k + 15 * 64 < nblocks:
            unrolled, k = True, k + 16 * 64
        tail = tail or k < nblocks
    return ('bn_partials_sum4', unrolled, tail)


def pool_reach(kernel, B, H, W, c):
    """maxpool / maxpool_idx / bn_relu_maxpool loop over the pooled float4 elements, maxpool_bwd over the un-pooled ones"""
    n = B * (H * W if kernel == 'maxpool_bwd' else pool_out(H) * pool_out(W)) * (c >> 2)
    return (kernel,) + _linear(n, capped_grid(n), 0)


def gap_bwd_reach(B, hw, c):
    n = B * hw * c
    return ('gap_bwd',) + _linear(n, capped_grid(n), 0)


# ------------------------------------------------------------------------------------------------------------------------------------
# case tables

# straps_bn_apply / _x3 / _bits_x3.  entry: 'plain' | 'x3' | 'bits'; y: write the fp32 output (False: y = NULL, planes only); planes: 0 none, 1 plane
# stride = rows * c rounded up to 8, 2 a stride larger than the extent
ApplyCase = namedtuple('ApplyCase', 'entry rows c res relu y planes')
APPLY = [
    ApplyCase('plain', 7, 96, False, False, True, 0),            # per_element, one trip
    ApplyCase('plain', 7, 96, True, True, True, 0),
    ApplyCase('plain', 43700, 96, True, True, True, 0),          # per_element past the cap
    ApplyCase('plain', 131072, 96, False, True, True, 0),        # per_element, exactly three trips for every thread
    ApplyCase('plain', 5, 64, True, False, True, 0),             # fixed, one partial trip
    ApplyCase('plain', 16, 64, False, True, True, 0),            # fixed, one whole trip
    ApplyCase('plain', 66537, 64, False, True, True, 0),         # fixed past the cap
    ApplyCase('plain', 131072, 64, True, False, True, 0),        # fixed, exactly two trips
    ApplyCase('x3', 5, 64, False, True, True, 1),
    ApplyCase('bits', 5, 64, True, True, False, 2),
    ApplyCase('x3', 16, 64, True, False, True, 0),
    ApplyCase('bits', 147, 128, False, True, True, 2),
    ApplyCase('x3', 147, 128, True, True, False, 1),
    ApplyCase('x3', 6, 768, True, True, True, 2),
    ApplyCase('bits', 6, 768, False, True, False, 1),
    ApplyCase('bits', 66537, 64, True, True, True, 1),           # fixed past the cap, with bit words
    ApplyCase('x3', 131072, 64, False, False, True, 0),
    ApplyCase('x3', 8, 256, False, False, True, 1),              # tiled, one trip
    ApplyCase('bits', 8, 256, True, True, False, 2),
    ApplyCase('bits', 5472, 768, True, True, True, 1),           # tiled, 4095-block grid (3 column blocks), past the cap
    ApplyCase('x3', 2068, 2048, False, True, False, 2),          # tiled, 8 column blocks, past the cap
    ApplyCase('bits', 32768, 256, False, True, True, 0),         # tiled, exactly two trips
]

# straps_bn_bwd and its forms.  entry: 'plain' (straps_bn_bwd) | 'x3' | 'bits' (_bits_x3) | 'finish' (_finish_x3) | 'finish_bits'; mask: 'none' | 'yact' |
# 'bits' | 'rederived' (mask_scale / mask_shift); flags: the accumulate word; dz: dz_out given; draw: the fp32 output given (False: planes only);
# planes as above; nblk: the partial blocks of the _finish forms (computed by the test in float64)
BwdCase = namedtuple('BwdCase', 'entry rows c mask flags dz draw planes nblk')
BWD = [
    BwdCase('plain', 9, 64, 'none', 0, True, True, 0, 0),                   # idle reduction rows
    BwdCase('plain', 9, 64, 'yact', 1, False, True, 0, 0),
    BwdCase('plain', 65, 4, 'rederived', 0, True, True, 0, 0),              # one active channel quad
    BwdCase('plain', 65, 4, 'yact', 2, True, True, 0, 0),
    BwdCase('plain', 64, 8, 'none', 3, True, True, 0, 0),                   # the unrolled loop alone
    BwdCase('x3', 130, 32, 'yact', 0, True, False, 2, 0),                   # tail loop only
    BwdCase('bits', 130, 32, 'bits', 1, False, True, 1, 0),
    BwdCase('finish', 130, 32, 'rederived', 3, True, True, 2, 65),
    BwdCase('finish_bits', 16, 64, 'bits', 0, False, True, 1, 1),           # apply pass: one whole trip
    BwdCase('plain', 131075, 4, 'yact', 0, True, True, 0, 0),               # 2048 blocks of 65 rows, trailing blocks empty, finalize past 1024 partials
    BwdCase('plain', 260160, 4, 'rederived', 1, False, True, 0, 0),         # blocks of 128 rows, the last one 64: no tail loop, trailing blocks empty
    BwdCase('bits', 140001, 64, 'bits', 0, False, True, 1, 0),              # unrolled loop plus tail, apply pass past the cap
    BwdCase('finish', 131072, 64, 'yact', 2, True, True, 0, 961),           # apply pass: exactly two trips
    BwdCase('x3', 8, 1024, 'rederived', 0, True, True, 1, 0),               # tiled, one trip
    BwdCase('finish_bits', 8, 1024, 'bits', 1, False, False, 2, 64),
    BwdCase('x3', 1372, 3072, 'yact', 0, False, False, 2, 0),               # tiled, 4092-block grid (12 column blocks), past the cap
    BwdCase('finish', 32768, 256, 'none', 0, False, True, 1, 1025),         # tiled, exactly two trips
    BwdCase('bits', 1373, 2048, 'bits', 3, False, True, 1, 0),              # fixed at 512 float4 channels (rows % 4 != 0)
    BwdCase('finish', 1373, 2048, 'none', 0, True, True, 0, 1),
]
FINISH_NBLK = (1, 64, 65, 961, 1025)

# one case per loop form, additionally against float64 autograd of F.batch_norm (+ ReLU): rows = B * H * H
AUTOGRAD = [(2, 3, 64), (2, 2, 1024), (1, 37, 2048)]            # (B, H, C): fixed; tiled; fixed at 512 float4 channels (1369 rows)

STATS_C = (1, 3, 6, 64, 130)
STATS_NBLOCKS = (1, 63, 64, 65, 960, 961, 1024, 1025, 2049)     # (1024: every lane group ends on a whole unrolled trip, no tail loop)

POOL_SMALL = [(1, 1, 1, 4), (2, 1, 9, 8), (1, 2, 2, 64), (1, 4, 4, 64), (3, 7, 8, 64), (1, 8, 7, 128), (1, 2, 2, 2048), (1, 3, 5, 2048)]      # B, H, W, C
POOL_FWD_BIG = (1, 257, 257, 256)
POOL_BWD_BIG = [(2, 182, 183, 64), (2, 256, 256, 64)]          # past the cap with a partial last POOL_CHUNK; exactly two trips of maxpool_bwd
POOL_SPARSE = (2, 7, 45, 64)                                    # W not a multiple of 32, H odd: ragged tiles on both edges

GAP_FWD = [(1, 1, 3), (5, 1, 130), (3, 49, 130), (2, 64, 3), (7, 33, 64)]        # batch, hw, c: c % 4 != 0, hw = 1, batch * c not a multiple of 256
GAP_BWD = [(1, 1, 3), (3, 49, 130), (5, 64, 3300), (8, 64, 4096), (2, 128, 128)]
MASKED_COPY = [(7, 33, 40, 35, 37), (1, 1, 1, 1, 1), (19, 130, 130, 131, 257), (256, 4, 4, 4, 4)]     # m, n, ldx, ldmask, ldy


def reached():
    got = set()
    for a in APPLY:
        got.add(bn_apply_reach('plain' if a.entry == 'plain' else 'x3', a.rows, a.c))
    for b in BWD:
        got.add(bn_bwd_apply_reach(b.rows, b.c))
        if b.entry in ('finish', 'finish_bits'):
            got.add(bn_partials_sum4_reach(b.nblk))
        else:
            got.add(bn_bwd_reduce_reach(b.rows, b.c))
            got.add(bn_partials_sum4_reach(straps_bn_bwd_blocks(b.rows, b.c)))
    for B, H, c in AUTOGRAD:
        got.add(bn_bwd_apply_reach(B * H * H, c))
    for n in STATS_NBLOCKS:
        got.add(bn_partials_sum4_reach(n))
    for s in POOL_SMALL + [POOL_FWD_BIG]:
        for k in ('maxpool', 'maxpool_idx', 'bn_relu_maxpool'):
            got.add(pool_reach(k, *s))
    for s in POOL_SMALL + POOL_BWD_BIG:
        got.add(pool_reach('maxpool_bwd', *s))
        got.add(bn_bwd_apply_pool_reach(*s))
    for s in GAP_BWD:
        got.add(gap_bwd_reach(*s))
    return got


_TT = tuple(itertools.product(('1', '>1'), (False, True)))
EVERY = set()
for _site, _forms in (('bn_apply', ('fixed', 'per_element')), ('bn_apply_x3', ('tiled', 'fixed', 'per_element')), ('bn_bwd_apply', ('tiled', 'fixed', 'per_element')),
                      ('bn_bwd_apply_pool', ('fixed', 'per_element')), ('maxpool', ('per_element',)), ('maxpool_idx', ('per_element',)),
                      ('bn_relu_maxpool', ('per_element',)), ('maxpool_bwd', ('per_element',)), ('gap_bwd', ('per_element',))):
    EVERY |= {(_site, f, t, tl) for f in _forms for (t, tl) in _TT}
EVERY |= {('bn_bwd_reduce', u, t, e) for u in (False, True) for t in (False, True) for e in (False, True)}
EVERY |= {('bn_partials_sum4', u, t) for u in (False, True) for t in (False, True)}

UNREACHABLE = {}
for _site in ('bn_apply_x3', 'bn_bwd_apply'):
    for _t, _tl in _TT:
        UNREACHABLE[(_site, 'per_element', _t, _tl)] = ('straps_grid256_rows makes grid x 256 a multiple of the row length C4 whenever m = C4 / gcd(C4, 256) <= 4096, and '
                                                        'both the cap and the rounded grid are multiples of m: true for every channel count of 4 .. 16384 with c % 4 == 0')
    UNREACHABLE[(_site, 'tiled', '1', True)] = ('the tiled form is chosen only for rows % (16 / wcg) == 0, and a grid under the cap is the whole number of tiles: '
                                                'every thread runs exactly one trip')
UNREACHABLE[('bn_apply', 'per_element', '1', False)] = 'one whole trip means n4 == grid x 256, and n4 = rows x C4 is a multiple of C4: that is the fixed form'
UNREACHABLE[('bn_bwd_apply_pool', 'per_element', '1', False)] = 'per_element needs C4 >= 512, one trip needs rows x C4 <= 256'
UNREACHABLE[('bn_bwd_apply_pool', 'per_element', '1', True)] = 'per_element needs C4 >= 512, one trip needs rows x C4 <= 256'
for _site in ('maxpool', 'maxpool_idx', 'bn_relu_maxpool'):
    UNREACHABLE[(_site, 'per_element', '>1', False)] = ('whole trips past the cap need a multiple of 2^20 pooled float4 elements, at least 2^21: an input of 33.5 million floats, '
                                                        'over the 20 million these tables allow a tensor')
UNREACHABLE[('bn_bwd_reduce', False, False, False)] = 'block 0 always has rows: one of the two loops runs'
UNREACHABLE[('bn_bwd_reduce', False, False, True)] = 'block 0 always has rows: one of the two loops runs'
UNREACHABLE[('bn_bwd_reduce', False, True, True)] = ('below the block cap nblk = ceil(rows / 64) and (nblk - 1) x ceil(rows / nblk) < rows: no empty block; at the cap rows > 64 x nblk, '
                                                     'so a block has at least 65 rows and the unrolled loop runs (tests/test_norm_cases_cpu.py sweeps this)')
UNREACHABLE[('bn_partials_sum4', False, False)] = 'nblocks > 0: lane group 0 always has a partial block'

assert set(UNREACHABLE) <= EVERY
REQUIRED = EVERY - set(UNREACHABLE)


def largest_tensor_floats():
    """the largest tensor (in 4-byte elements) any case of the tables hands to or gets from a kernel"""
    sizes = [a.rows * a.c for a in APPLY] + [b.rows * b.c for b in BWD] + [B * H * H * c for B, H, c in AUTOGRAD]
    sizes += [B * H * W * c for B, H, W, c in POOL_SMALL + [POOL_FWD_BIG, POOL_SPARSE] + POOL_BWD_BIG]
    sizes += [max(b.nblk, straps_bn_bwd_blocks(b.rows, b.c)) * b.c * 4 for b in BWD]            # partials: doubles, two per channel
    sizes += [n * c * 2 for n in STATS_NBLOCKS for c in STATS_C]
    sizes += [b * hw * c for b, hw, c in GAP_FWD + GAP_BWD] + [m * max(ldx, ldm, ldy) for m, n, ldx, ldm, ldy in MASKED_COPY]
    return sizes
